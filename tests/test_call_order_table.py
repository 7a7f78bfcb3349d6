"""CPU: the family table of tests/test_gpu_call_order.py is complete.  Every export of
`_lib.SIGNATURES` is a key of FAMILIES (it takes memory from the handle, and a row runs it behind
every predecessor state) or a member of NO_HANDLE_MEMORY with the reason of its group; a new
export fails here until someone classifies it.  Reads the two tables only."""
import test_gpu_call_order as co


def test_every_export_is_classified():
    from pb_bss_amd import _lib
    exports = set(_lib.SIGNATURES)
    table = set(co.FAMILIES)
    exempt = set().union(*co.NO_HANDLE_MEMORY.values())
    assert sum(len(group) for group in co.NO_HANDLE_MEMORY.values()) == len(exempt), \
        'an export sits in two groups of NO_HANDLE_MEMORY'
    assert all(len(reason.split()) >= 3 for reason in co.NO_HANDLE_MEMORY), 'a group needs a reason'
    assert not table & exempt, sorted(table & exempt)
    assert not (table | exempt) - exports, sorted((table | exempt) - exports)   # no stale names
    missing = exports - table - exempt
    assert not missing, (
        f'{sorted(missing)}: add a row to ROWS of tests/test_gpu_call_order.py if the export '
        'takes memory from the handle (work / scratch slab, xbuf, team buffer), or name it in '
        'NO_HANDLE_MEMORY with the reason')


def test_rows_are_well_formed():
    for name, row in co.ROWS.items():
        assert row.exports and set(row.shape) == {'small', 'big'}, name
        assert len(row.seeds) == 2 and row.seeds[0] != row.seeds[1], name
        assert callable(row.oracle) and callable(row.poison) and callable(row.run), name
        assert (row.timeout is None) or callable(row.timeout), name
    # the rows that wait between workgroups are run behind a consumed time-out; the packed-FP32
    # split groups cannot be made to give up (test_after_a_time_out_that_the_engine_consumed)
    assert set(co.TIMEOUT_ROWS) == {'em_split', 'em_shared', 'cwmm_split', 'dhtv_team_2',
                                    'dhtv_team_-2'}
    assert all(isinstance(co.ROWS[n].timeout.match, str) for n in co.TIMEOUT_ROWS)
    assert set(co.TIMEOUT_ROWS) | {'em_split_f32'} <= set(co.XBUF_ROWS)
    assert not set(co.NOT_REPRODUCIBLE) - set(co.ROWS)
