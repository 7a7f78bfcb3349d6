// extern "C" boundary of the multi-GPU helpers (include/pbbss.h; RCCL communicator in the handle
// and the mask all-gather: comm.hip) and of pbbss_normalize_observation: argument validation and
// the gather buffers.  No device code lives here.
#include "handle.hpp"
#include "beamform.hpp"
#include "comm.hpp"

using pbbss::as_stream, pbbss::Carver, pbbss::carve, pbbss::DeviceGuard;

PBBSS_API int pbbss_comm_unique_id(void* out_id) {
  if (!out_id) return PBBSS_ERR_INVALID_ARG;
  return pbbss::comm_unique_id(out_id);
}

PBBSS_API int pbbss_comm_create(pbbss_handle_t h, const void* unique_id, int world_size, int rank) {
  DeviceGuard device_guard(h);
  if (!h || !unique_id || world_size < 1 || rank < 0 || rank >= world_size)
    return PBBSS_ERR_INVALID_ARG;
  if (h->comm) return PBBSS_ERR_INVALID_ARG;  // one communicator per handle
  void* c = nullptr;
  const int rc = pbbss::comm_create(unique_id, world_size, rank, &c);
  if (rc != PBBSS_OK) return rc;
  h->comm = c;
  h->comm_world = world_size;
  h->comm_rank = rank;
  return PBBSS_OK;
}

PBBSS_API int pbbss_comm_destroy(pbbss_handle_t h) {
  DeviceGuard device_guard(h);
  if (!h) return PBBSS_ERR_INVALID_ARG;
  // collectives enqueued on any stream of this device finish before their buffers go away
  if (h->comm) (void)hipDeviceSynchronize();
  const int rc = pbbss::comm_destroy(h->comm);
  h->comm = nullptr;
  h->comm_world = 1;
  h->comm_rank = 0;
  h->comm_buf.release();
  return rc;
}

PBBSS_API int pbbss_comm_info(pbbss_handle_t h, int* out_world_size, int* out_rank) {
  if (!h || !out_world_size || !out_rank) return PBBSS_ERR_INVALID_ARG;
  if (!h->comm) return PBBSS_ERR_INVALID_ARG;  // pbbss_comm_create first
  return pbbss::comm_query(h->comm, out_world_size, out_rank);
}

PBBSS_API int pbbss_shard_bounds(int64_t total_bins, int world_size, int rank, int64_t* out_start,
                                 int64_t* out_stop) {
  if (total_bins < 0 || world_size < 1 || rank < 0 || rank >= world_size || !out_start || !out_stop)
    return PBBSS_ERR_INVALID_ARG;
  const int64_t base = total_bins / world_size, extra = total_bins % world_size;
  *out_start = rank * base + (rank < extra ? rank : extra);
  *out_stop = *out_start + base + (rank < extra ? 1 : 0);
  return PBBSS_OK;
}

PBBSS_API int pbbss_allgather_unpack(pbbss_handle_t h, const void* gathered, int elem_bytes,
                                     int world_size, int64_t outer, int64_t total_bins,
                                     int64_t inner, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !gathered || !out || world_size < 1 || outer < 0 || total_bins < 0 || inner < 0)
    return PBBSS_ERR_INVALID_ARG;
  if (elem_bytes != 4 && elem_bytes != 8) return PBBSS_ERR_UNSUPPORTED;
  return pbbss::launch_allgather_unpack(gathered, elem_bytes, world_size, outer, total_bins, inner,
                                        out, as_stream(stream));
}

PBBSS_API int pbbss_allgather_masks(pbbss_handle_t h, const void* local, int elem_bytes,
                                    int64_t outer, int64_t total_bins, int64_t inner, void* out,
                                    void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !out || outer < 0 || total_bins < 0 || inner < 0) return PBBSS_ERR_INVALID_ARG;
  if (elem_bytes != 4 && elem_bytes != 8) return PBBSS_ERR_UNSUPPORTED;
  if (!h->comm) return PBBSS_ERR_INVALID_ARG;  // pbbss_comm_create first
  const int world = h->comm_world;
  int64_t lo = 0, hi = 0;
  (void)pbbss_shard_bounds(total_bins, world, h->comm_rank, &lo, &hi);
  const int64_t nloc = hi - lo, pad = (total_bins + world - 1) / world;
  if (nloc > 0 && !local) return PBBSS_ERR_INVALID_ARG;
  const size_t block = (size_t)outer * pad * inner * elem_bytes;
  if (block == 0) return PBBSS_OK;
  // The pack / gather buffers belong to the communicator (grow-only, released by
  // pbbss_comm_destroy / pbbss_destroy): the work slab may be re-carved or reallocated by the next
  // library call on another stream while this collective is still in flight.
  char *packed, *gathered;
  int rc = carve(h->comm_buf, [&](Carver& wc) {
    packed = wc.take<char>(block);
    gathered = wc.take<char>(block * world);
  });
  if (rc != PBBSS_OK) return rc;
  hipStream_t s = as_stream(stream);
  rc = pbbss::launch_allgather_pack(local, elem_bytes, outer, nloc, pad, inner, packed, s);
  if (rc != PBBSS_OK) return rc;
  rc = pbbss::comm_all_gather_bytes(h->comm, packed, gathered, block, s);
  if (rc != PBBSS_OK) return rc;
  return pbbss::launch_allgather_unpack(gathered, elem_bytes, world, outer, total_bins, inner, out,
                                        s);
}

PBBSS_API int pbbss_normalize_observation(pbbss_handle_t h, const void* y, int is_c128,
                                          int64_t B, int T, int D, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !out || B <= 0 || T <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  for (int64_t b0 = 0; b0 < B; b0 += 65535) {  // grid.y limit: split the batch
    int64_t nb = (B - b0 < 65535) ? (B - b0) : 65535;
    size_t esz = is_c128 ? 16 : 8;
    int rc = pbbss::launch_normalize((const char*)y + (size_t)b0 * T * D * esz, is_c128, nb, T, D,
                                     (char*)out + (size_t)b0 * T * D * esz, as_stream(stream));
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}
