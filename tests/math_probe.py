"""ctypes loader of lib/libnngp_mathprobe.so (tests/probe/nngp_math_probe.hip, built by csrc/Makefile
beside the product library): the device routines of csrc/nngp_math.h over arrays.  Test
infrastructure; a missing library is an error (OSError), never a skip."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, 'nearest-neighbors-gparareal_amd', 'lib', 'libnngp_mathprobe.so')

# the `fn` codes of tests/probe/nngp_math_probe.hip
FN = {'nn_exp': 0, 'nn_exp_nonpos': 1, 'nn_exp_nonpos_sep': 2, 'nn_exp_dd': 3, 'nn_pow10': 4, 'nn_log': 5,
      'nn_sincos': 6, 'nn_sin': 7, 'nn_cos': 8, 'nn_sin_pi': 9, 'sqrt_mid': 10, 'rcp_mid': 11,
      'in_mid_range': 12, 'sqrt_rcp_exact': 13}
TWO_OUTPUTS = ('nn_sincos', 'sqrt_mid', 'rcp_mid', 'sqrt_rcp_exact')

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB_PATH)
        L.nngp_math_probe.argtypes = [ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 5
        L.nngp_math_probe.restype = ctypes.c_int
        _lib = L
    return _lib


SENTINEL = -7.0


def run(name, a, b=None):
    """The routine `name` over the float64 array a (and b: nn_exp_dd's lo) on the current device:
    (out0, out1) as numpy arrays, out1 None for the one-output routines.  Bits travel unchanged."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = a.size
    at = torch.from_numpy(a.copy()).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64).copy()).cuda() if b is not None else None
    assert bt is None or bt.numel() == n
    out0 = torch.full((n,), SENTINEL, dtype=torch.float64, device='cuda')
    out1 = torch.full((n,), SENTINEL, dtype=torch.float64, device='cuda') if name in TWO_OUTPUTS else None
    rc = lib().nngp_math_probe(FN[name], n, at.data_ptr(), bt.data_ptr() if bt is not None else None,
                               out0.data_ptr(), out1.data_ptr() if out1 is not None else None,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, f'nngp_math_probe({name}): HIP error {rc}'
    return out0.cpu().numpy(), (out1.cpu().numpy() if out1 is not None else None)
