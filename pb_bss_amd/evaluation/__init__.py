"""Drop-in for pb_bss.evaluation (reference: pb_bss/evaluation/__init__.py) on the device:
`si_sdr`, the `sxr_module` (`get_snr`, `set_snr`, `input_sxr`, `output_sxr`), the BSS-Eval
metrics `mir_eval_sources` (SDR / SIR / SAR, computed here without the `mir_eval` package),
`srmr` (the reference's own NumPy / SciPy code, restated for the device; it needs no clean
source) and the `InputMetrics` / `OutputMetrics` classes.

The reference's `pesq` wraps a third-party package and is not provided; `stoi` is computed here
without the `pystoi` package.  The two classes list `pesq` and `stoi`, and for now `srmr` too,
as disabled and raise NotImplementedError for them."""
from . import sxr_module
from .module_mir_eval import mir_eval_sources
from .module_si_sdr import si_sdr
from .module_srmr import srmr
from .module_stoi import stoi
from .wrapper import InputMetrics, OutputMetrics

__all__ = ['si_sdr', 'sxr_module', 'mir_eval_sources', 'srmr', 'stoi', 'InputMetrics',
           'OutputMetrics']
