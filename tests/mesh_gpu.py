"""What the GPU suites of the mesh operations (tests/test_gpu_mesh_components.py, _simplify, _smooth, _holes, _closest, _rays) share to
make a raw C-ABI call and to compare its outputs: pointers, the current stream, uploads and bit comparisons.  A plain module, imported
like mesh_ref; it holds no test and needs a GPU only where a function is called."""
import ctypes as C

import numpy as np
import torch

F32 = np.float32


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_tri(tri):
    return torch.from_numpy(np.ascontiguousarray(tri, np.uint32).view(np.int32).reshape(-1, 3)).cuda()


def dev_vtx(v):
    return torch.from_numpy(np.ascontiguousarray(v, F32).reshape(-1, 4)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def same_or_both_nan(got_u32, want_f32):
    """Bit-equal, except that wherever the restatement has a NaN the GPU has a NaN (payloads differ between x86 and the GPU)."""
    got = got_u32.view(F32)
    nan = np.isnan(want_f32)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got_u32[~nan], want_f32.view(np.uint32)[~nan])
