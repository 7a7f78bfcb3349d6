"""Drop-in for the NumPy part of pb_bss.evaluation (reference: pb_bss/evaluation/__init__.py):
`si_sdr` and the `sxr_module` (`get_snr`, `set_snr`, `input_sxr`, `output_sxr`) on the device.

The reference's other metrics (`mir_eval_sources`, `pesq`, `stoi`, `srmr`) and the
`InputMetrics` / `OutputMetrics` classes on top of them wrap third-party packages and are not
provided."""
from . import sxr_module
from .module_si_sdr import si_sdr

__all__ = ['si_sdr', 'sxr_module']
