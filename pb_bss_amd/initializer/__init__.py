"""Initialisations for the mixture-model trainers (reference package: pb_bss/initializer).

    from pb_bss_amd.initializer import deflation, iid, deterministic
    seed = deflation.deflationSeed(Y, 3)                      # (K, F, T), on the device
    model = CACGMMTrainer().fit(Y, initialization=seed.transpose(1, 0, 2), iterations=100)
"""
from . import iid  # noqa: F401
from . import deflation  # noqa: F401
from . import deterministic  # noqa: F401
