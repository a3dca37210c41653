"""tests/_e4m3.py on the CPU: the NumPy quantiser against torch's float8_e4m3fn conversion on every bf16 bit pattern, the share of
elements with two admissible bytes, the checker's teeth (five planted mutations, each reported) and its soundness (an fp32 tensor's
direct e4m3 rounding always passes against the tensor's bf16 rounding)."""
import numpy as np
import pytest
import torch

import _e4m3 as E

FP8 = torch.float8_e4m3fn


def _all_bf16():
    """all 2^16 bf16 bit patterns as a bf16 tensor"""
    return torch.arange(1 << 16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


@pytest.mark.parametrize("scale", [None, 2.0 ** 17, 2.0 ** -9, 3.0, 0.3])
def test_quantize_ref_equals_torch_on_all_bf16(scale):
    x = _all_bf16().float()
    got = E.quantize_ref(x, scale)
    xs = x if scale is None else x * torch.tensor(scale, dtype=torch.float32)
    want = xs.clamp(-448.0, 448.0).to(FP8).view(torch.uint8).numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    nan, inf = torch.isnan(xs).numpy(), torch.isinf(xs).numpy()
    sign = np.signbit(xs.numpy())
    assert nan.sum() >= 254 and np.array_equal(got[nan], np.where(sign[nan], 0xFF, 0x7F))
    assert inf.sum() >= 2 and np.array_equal(got[inf], np.where(sign[inf], 0xFE, 0x7E))


def test_table_is_the_format():
    assert E.TABLE.size == 127 and E.TABLE[0] == 0 and E.TABLE[1] == 2.0 ** -9 and E.TABLE[8] == 2.0 ** -6 and E.TABLE[126] == 448.0
    assert (np.diff(E.TABLE) > 0).all()
    back = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(FP8).float().double().numpy()
    mine = E.decode(np.arange(256, dtype=np.uint8))
    assert np.array_equal(np.isnan(back), np.isnan(mine)) and np.array_equal(back[~np.isnan(back)], mine[~np.isnan(mine)])


def test_two_byte_share():
    """8 of the 128 bf16 values of a binade are e4m3 rounding boundaries (the odd multiples of 2^-4 of the binade's base): 1 / 16."""
    bits = (np.arange(128) | (127 << 7)).astype(np.uint16)           # [1, 2)
    b = torch.from_numpy(bits.astype(np.int16)).view(torch.bfloat16).float().numpy()
    lo, hi = E.admissible(b, 1.0)
    assert int((lo != hi).sum()) == 8
    assert np.array_equal(b[lo != hi], 1 + (2 * np.arange(8) + 1) / 16)
    # the same binade moved into the subnormal range of e4m3: boundaries are odd multiples of 2^-10
    lo, hi = E.admissible(b, 2.0 ** -8)                               # [2^-8, 2^-7): bytes 2 .. 4, boundaries 2.5 and 3.5 (x 2^-9)
    assert int((lo != hi).sum()) == 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 10, 1 << 10, generator=g).to(torch.bfloat16)
    st = E.check_image(E.quantize_ref(x.float()), x, 1.0, "randn")
    # 1 / 16 if a binade's 128 values were equally likely; the normal density tilts each binade a little (0.0622 measured)
    assert 0.055 < st["two_byte"] < 0.070, st
    assert st["saturated"] == 0 and st["subnormal"] > 1000 and st["nan"] == 0


def _image(seed=1, rows=64, cols=256, scale=2.0 ** 8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-18, 2, (rows, cols), generator=g).float())
    b = x.to(torch.bfloat16)
    img = E.quantize_ref(b.float(), scale)
    st = E.check_image(img, b, scale, "clean")
    assert st["saturated"] >= 100 and st["subnormal"] >= 100 and st["zero"] >= 100, st
    return b, img, scale


def test_checker_reports_swapped_chunks():
    b, img, s = _image()
    m = img.copy()
    m[5, 32:48], m[5, 96:112] = img[5, 96:112], img[5, 32:48]
    with pytest.raises(AssertionError, match=r"2 16-byte chunks in 1 rows affected \(rows \[5\]\).*displacement: 2 of the first 2 bad chunks"):
        E.check_image(m, b, s, "swap")


def test_checker_reports_copied_row():
    b, img, s = _image()
    m = img.copy()
    m[9] = img[40]
    with pytest.raises(AssertionError, match=r"in 1 rows affected \(rows \[9\]\).*1 of the first 1 bad rows hold another row's expected bytes"):
        E.check_image(m, b, s, "row copy")


def test_checker_reports_one_truncated_element():
    b, img, s = _image()
    y = b.float().numpy().astype(np.float64) * s
    mag = img & 0x7F
    # an element that rounded UP, not on a boundary, not saturated: truncation gives the byte below
    up = (E.TABLE[np.minimum(mag, 126)] > np.abs(y)) & (mag > 1) & (mag < 0x7E)
    lo, hi = E.admissible(b, s)
    up &= lo == hi
    r, c = (int(v[0]) for v in np.nonzero(up))
    m = img.copy()
    m[r, c] -= 1
    with pytest.raises(AssertionError, match=rf"trunc: 1 of {img.size} e4m3 bytes.*first at \(row {r}, col {c}\): got 0x{m[r, c]:02X}, want 0x{img[r, c]:02X} "):
        E.check_image(m, b, s, "trunc")


def test_checker_reports_nan_byte_in_place_of_saturation():
    b, img, s = _image()
    r, c = (int(v[0]) for v in np.nonzero(img == 0x7E))
    m = img.copy()
    m[r, c] = 0x7F
    with pytest.raises(AssertionError, match=r"got 0x7F, want 0x7E .*1 bad bytes are NaN bytes"):
        E.check_image(m, b, s, "nan for 448")
    r, c = (int(v[0]) for v in np.nonzero(img == 0xFE))
    m = img.copy()
    m[r, c] = 0xFF
    with pytest.raises(AssertionError, match=r"got 0xFF, want 0xFE "):
        E.check_image(m, b, s, "nan for -448")


def test_checker_reports_image_of_twice_the_tensor():
    b, img, s = _image()
    m = E.quantize_ref(2 * b.float(), s)
    with pytest.raises(AssertionError) as e:
        E.check_image(m, b, s, "2b")
    n_bad = int(str(e.value).split(":")[1].split()[0])
    # every element that is neither zero nor saturated before and after moves by eight bytes
    assert n_bad > 0.7 * img.size, str(e.value)


def test_checker_nan_and_signed_zero_rules():
    b = torch.tensor([[float("nan"), -float("nan"), 0.0, -0.0, 2.0 ** -12, -2.0 ** -12, 2.0 ** -10, -2.0 ** -10, 1e9, -1e9,
                       float("inf"), -float("inf"), 1.0625, -1.0625, 448.0, 432.0]], dtype=torch.float32).to(torch.bfloat16)
    b.view(torch.int16)[0, :2] = torch.tensor([0x7FC0, 0xFFC0 - (1 << 16)], dtype=torch.int16)      # the NaNs by their bits
    lo, hi = E.admissible(b, 1.0)
    assert lo.tolist() == [[0x7F, 0xFF, 0x80, 0x80, 0x80, 0x80, 0x80, 0x81, 0x7E, 0xFE, 0x7E, 0xFE, 0x38, 0xB9, 0x7E, 0x7D]]
    assert hi.tolist() == [[0x7F, 0xFF, 0x00, 0x00, 0x00, 0x00, 0x01, 0x00, 0x7E, 0xFE, 0x7E, 0xFE, 0x39, 0xB8, 0x7E, 0x7E]]
    img = E.quantize_ref(b.float())
    assert img.tolist() == [[0x7F, 0xFF, 0x00, 0x80, 0x00, 0x80, 0x00, 0x80, 0x7E, 0xFE, 0x7E, 0xFE, 0x38, 0xB8, 0x7E, 0x7E]]
    st = E.check_image(img, b, 1.0, "rules")
    assert st == {"n": 16, "two_byte": 5 / 16, "saturated": 6, "subnormal": 0, "zero": 6, "nan": 2}
    for col, byte in ((0, 0xFF), (0, 0x7E), (0, 0xFE), (2, 0x01), (8, 0x7F), (12, 0x3A), (14, 0x7D)):
        m = img.copy()
        m[0, col] = byte
        with pytest.raises(AssertionError, match=rf"first at \(row 0, col {col}\): got 0x{byte:02X}"):
            E.check_image(m, b, 1.0, "rules")


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 17, 2.0 ** -9])
def test_direct_rounding_always_passes(scale):
    """v fp32, b = bf16(v), image = e4m3(v scale) rounded directly: inside the admissible pair of b, whatever v is."""
    g = torch.Generator().manual_seed(int(np.log2(scale)) + 100)
    n = 1000 * 1000
    # magnitudes from below the smallest subnormal's boundary (2^-10) to beyond 448, all after the scale
    v = torch.randn(n, generator=g) * torch.exp2(torch.randint(-13, 10, (n,), generator=g).float()) / scale
    # and values planted right beside boundaries: a boundary +- a few fp32 steps rounds to the boundary in bf16
    mids = torch.from_numpy(E.MID).float()
    k = torch.randint(0, mids.numel(), (n // 10,), generator=g)
    off = torch.randint(-3, 4, (n // 10,), generator=g, dtype=torch.int32)
    near = (mids[k].view(torch.int32) + off).view(torch.float32) / scale
    near = near * (1 - 2 * torch.randint(0, 2, (n // 10,), generator=g)).float()
    v = torch.cat([v[: n - near.numel()], near]).view(1000, 1000)
    b = v.to(torch.bfloat16)
    st = E.check_image(E.quantize_ref(v, scale), b, scale, f"direct rounding, scale {scale}")
    assert st["saturated"] > 1000 and st["subnormal"] > 1000 and st["zero"] > 1000 and st["two_byte"] > 0.1, st
