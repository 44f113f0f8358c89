"""The host mirror's image layout (no GPU): dynamicfusion_amd.tsdf_volume._image turns a tensor into the C-ABI's (pointer, byte pitch,
rows, cols) -- dense tensors keep the pitch they always had, column windows and row bands of wider images pass their own row stride --
and refuses every layout the ABI cannot express (include/dfusion.h: one byte pitch per image, dense pixels within a row)."""
import pytest
import torch

from dynamicfusion_amd.tsdf_volume import BGRA, F4, U16, _flat, _image


def img(t, kind):
    p, pitch, rows, cols = _image(t, kind, check_device=False)
    assert p.value == t.data_ptr()
    return pitch, rows, cols


def test_dense_tensors_keep_their_pitch():
    assert img(torch.zeros((117, 203), dtype=torch.int16), U16) == (203 * 2, 117, 203)
    assert img(torch.zeros((480, 640, 4), dtype=torch.float32), F4) == (640 * 16, 480, 640)
    assert img(torch.zeros((117, 203, 4), dtype=torch.uint8), BGRA) == (203 * 4, 117, 203)
    assert img(torch.zeros((1, 8, 4), dtype=torch.float32), F4) == (8 * 16, 1, 8)           # one row: the dense pitch


def test_column_windows_and_row_bands_pass_their_row_stride():
    wide = torch.zeros((480, 1000), dtype=torch.int16)
    assert img(wide[:, 40:360], U16) == (1000 * 2, 480, 320)
    assert img(wide[:, 1:204], U16) == (1000 * 2, 480, 203)                                    # odd x0: rows not 4-byte aligned
    assert img(wide[::2], U16) == (2000 * 2, 240, 1000)                                        # every other row
    assert img(wide[100:164], U16) == (1000 * 2, 64, 1000)                                     # a row band: dense, same pitch
    w4 = torch.zeros((240, 330, 4), dtype=torch.float32)
    assert img(w4[:, 1:321], F4) == (330 * 16, 240, 320)
    assert img(w4[10:20, 5:9], F4) == (330 * 16, 10, 4)
    wb = torch.zeros((50, 70, 4), dtype=torch.uint8)
    assert img(wb[:, 3:40], BGRA) == (70 * 4, 50, 37)


def test_wrong_dtype_or_shape_is_refused():
    for t, kind in ((torch.zeros((4, 8), dtype=torch.float32), U16), (torch.zeros((4, 8), dtype=torch.int32), U16),
                    (torch.zeros((4, 8, 4), dtype=torch.float64), F4), (torch.zeros((4, 8, 4), dtype=torch.float32), BGRA),
                    (torch.zeros((4, 8, 3), dtype=torch.float32), F4), (torch.zeros((4, 32), dtype=torch.float32), F4),
                    (torch.zeros((4, 8, 4), dtype=torch.int16), U16)):
        with pytest.raises(ValueError):
            _image(t, kind, check_device=False)


def test_non_dense_rows_are_refused():
    d = torch.zeros((64, 80), dtype=torch.int16)
    f = torch.zeros((64, 80, 4), dtype=torch.float32)
    for t, kind in ((d.t(), U16),                                                  # transposed: stride(-1) != 1
                    (d[:, ::2], U16),                                              # every other column
                    (f[:, ::2], F4),                                               # stride(1) != 4
                    (f.permute(1, 0, 2), F4),                                      # transposed float4
                    (d.as_strided((64, 80), (40, 1)), U16),                        # rows overlap: stride(0) < one row
                    (d.unsqueeze(0).expand(3, 64, 80)[:, 0], U16)):                # stride(0) == 0: every row the same memory
        with pytest.raises(ValueError):
            _image(t, kind, check_device=False)


def test_negative_row_stride_is_refused():
    d = torch.zeros((64, 80), dtype=torch.int16)
    neg = type("Neg", (), {})()                       # torch has no negative strides; the check still has to be there for views that do
    neg.dtype, neg.is_cuda, neg.shape = torch.int16, True, (64, 80)
    neg.dim = lambda: 2
    neg.stride = lambda i=None: (-80, 1) if i is None else (-80, 1)[i]
    neg.element_size = lambda: 2
    neg.data_ptr = lambda: d.data_ptr() + 63 * 160
    with pytest.raises(ValueError):
        _image(neg, U16)


def test_misaligned_float4_is_refused():
    buf = torch.zeros((32, 40 * 4 + 8), dtype=torch.float32)
    ok = buf[:, 4:4 + 80].unflatten(1, (20, 4))                                     # x0 = one pixel: aligned
    assert img(ok, F4) == ((40 * 4 + 8) * 4, 32, 20)
    with pytest.raises(ValueError):
        _image(buf[:, 1:1 + 80].unflatten(1, (20, 4)), F4, check_device=False)      # x0 not a whole pixel: base 4 bytes off
    odd = torch.zeros((32, 40 * 4 + 2), dtype=torch.float32)
    with pytest.raises(ValueError):
        _image(odd[:, :80].unflatten(1, (20, 4)), F4, check_device=False)           # row pitch not a multiple of 16 bytes
    b = torch.zeros((16, 41 * 4 + 1), dtype=torch.uint8)
    with pytest.raises(ValueError):
        _image(b[:, 1:81].unflatten(1, (20, 4)), BGRA, check_device=False)          # BGRA stored as 32-bit words


def test_host_tensor_is_refused():
    with pytest.raises(ValueError):
        _image(torch.zeros((4, 8), dtype=torch.int16), U16)


def test_flat_lists_must_be_contiguous():
    p = torch.zeros((100, 4), dtype=torch.float32)
    assert _flat(p).value == p.data_ptr() and _flat(p[10:20]).value == p[10:20].data_ptr()
    for t in (p[::2], p[:, :3], p.t()):
        with pytest.raises(ValueError):
            _flat(t)
