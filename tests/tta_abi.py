"""The five skp_tta_reduce* entry points as the CPU tests call them through the C ABI: one valid
argument tuple each, whose pointers are an aligned non-null dummy, so that a call with one argument
made bad fails its check before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

A = ctypes.c_void_p(256)
R2 = float(np.float32((0.05 * 37) ** 2))

# entry point -> (valid arguments, the slots of its required pointers, the workspace's last)
ENTRY_POINTS = {
    #                         maps B  C  n  S  theta
    "skp_tta_reduce":         ((A, 2, 3, 5, 37, A, A, None, A, None), (0, 5, 6, 8)),                       # pos avg ws stream
    "skp_tta_reduce_scored":  ((A, 2, 3, 5, 37, A, 5.0, A, A, A, None, A, None), (0, 5, 7, 8, 9, 11)),     # dist pos ref scores …
    "skp_tta_reduce_peaks":   ((A, 2, 3, 5, 37, A, 3, R2, A, A, None, A, None), (0, 5, 8, 9, 11)),         # num r2 pos values …
    "skp_tta_reduce_entropy": ((A, 2, 3, 5, 37, A, 1.0, A, A, None, A, None), (0, 5, 7, 8, 10)),           # scale pos entropy …
    "skp_tta_reduce_parts":   ((A, 2, 3, 5, 37, A, A, A, A, A, None, A, None), (0, 5, 6, 7, 8, 9, 11)),    # pos label value mass …
}


def library():
    from stablekeypoints_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libskp.so not built")
    return _lib.lib()


def rc_with(L, entry, **kw):
    """``entry``'s return code on its valid arguments with slot i replaced by v for every ``a<i>=v``."""
    args = list(ENTRY_POINTS[entry][0])
    for k, v in kw.items():
        args[int(k[1:])] = v
    return getattr(L, entry)(*args)
