"""OCP e4m3fn on the host, restated from the format's definition (no torch conversion), and a per-element judge of the e4m3
images that kernels write beside their bf16 outputs.

Format: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinity; 0x7F / 0xFF are NaN.  Byte b < 0x7F is
    (b & 7) 2^-9                      for b < 8          (subnormal)
    (8 + (b & 7)) 2^((b >> 3) - 10)    otherwise,         up to 0x7E = 448.
The kernels saturate: everything at or beyond +-448, the infinities included, is +-448; NaN stays NaN and keeps its sign.

`admissible`: a kernel turns an fp32 value v into both images; the test sees b = bf16(v).  Rounding to bf16 is monotone and
every e4m3 rounding boundary m (a midpoint of two neighbouring bytes: 5 significant bits) is a bf16 value, so v < m implies
b <= m, and b != m implies b < m: unless b sits exactly ON a boundary, v and b lie on the same side of every boundary and the byte
is the quantisation of b.  On a boundary v may have been on either side, so both neighbours are admitted.  A power-of-two scale
moves b and the boundaries together."""
import numpy as np

MAXV = 448.0
NAN_BYTE = 0x7F
# the 127 non-negative finite values, byte order = value order
TABLE = np.array([(b & 7) * 2.0 ** -9 if b < 8 else (8 + (b & 7)) * 2.0 ** ((b >> 3) - 10) for b in range(127)], dtype=np.float64)
MID = (TABLE[:-1] + TABLE[1:]) / 2          # MID[i] between bytes i and i + 1: exact in fp64
SUB_MAX_BYTE = 7                             # bytes 1..7 are subnormal


def _np(x, dtype=None):
    if hasattr(x, "detach"):
        import torch
        x = x.detach().cpu()
        if x.dtype in (torch.bfloat16, torch.float16):
            x = x.float()
        elif x.dtype == torch.float8_e4m3fn:
            x = x.view(torch.uint8)
        x = x.numpy()
    x = np.asarray(x)
    return x.astype(dtype) if dtype is not None and x.dtype != dtype else x


def decode(b8):
    """bytes -> fp64 values (NaN bytes -> NaN)"""
    b8 = _np(b8, np.uint8)
    mag = b8 & 0x7F
    v = np.where(mag == 0x7F, np.nan, TABLE[np.minimum(mag, 126)])
    return np.where(b8 & 0x80, -v, v)


def _scaled(x32, scale):
    x = _np(x32, np.float32)
    if scale is None:
        return x
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return x * np.float32(scale)            # one fp32 multiply, as the kernels do


def _magnitude_bytes(a):
    """a: fp64 magnitudes, no NaN, already clamped to 448 -> (byte, on a boundary, lower neighbour).  Round to nearest, ties to
    the even byte."""
    lo = np.searchsorted(MID, a, side="left")             # number of boundaries strictly below a: the byte unless a is ON one
    on = (lo < MID.size) & (MID[np.minimum(lo, MID.size - 1)] == a)
    byte = np.where(on, lo + (lo & 1), lo)                 # a == MID[lo]: between bytes lo and lo + 1, take the even one
    return byte.astype(np.uint8), on, lo.astype(np.uint8)


def quantize_ref(x32, scale=None):
    """e4m3fn bytes (uint8 array of x32's shape) of fp32 values, after one fp32 multiply by `scale` if given."""
    y = _scaled(x32, scale)
    nan = np.isnan(y)
    sign = np.where(np.signbit(y), 0x80, 0).astype(np.uint8)
    a = np.minimum(np.abs(np.where(nan, 0, y)).astype(np.float64), MAXV)
    byte, _, _ = _magnitude_bytes(a)
    return np.where(nan, NAN_BYTE, byte).astype(np.uint8) | sign


def key(b8):
    """bytes in value order: -NaN -128, -448 -127, ..., -0 -1, +0 0, ..., 448 126, NaN 127"""
    b = _np(b8, np.uint8).astype(np.int16)
    return np.where(b < 0x80, b, 0x7F - b)


def admissible(b_bf16, scale=1.0):
    """(lo, hi): per element the lowest and the highest admissible byte, in value order, of the e4m3 image of a value whose bf16
    image is `b_bf16`, under the power-of-two `scale`."""
    m, e = np.frexp(float(scale))
    assert m == 0.5, f"scale {scale} is not a power of two"
    y = _scaled(b_bf16, scale)
    nan = np.isnan(y)
    neg = np.signbit(y)
    a = np.minimum(np.abs(np.where(nan, 0, y)).astype(np.float64), MAXV)
    byte, on, below = _magnitude_bytes(a)
    small = np.where(on, below, byte).astype(np.uint8)         # in magnitude
    large = np.where(on, below + 1, byte).astype(np.uint8)
    sign = np.where(neg, 0x80, 0).astype(np.uint8)
    lo = np.where(neg, large, small) | sign                   # value order: the larger magnitude is the lower negative value
    hi = np.where(neg, small, large) | sign
    # a zero result (b is +-0, or the value underflows): +0 and -0 are the same number
    lo = np.where((lo & 0x7F) == 0, 0x80, lo)
    hi = np.where((hi & 0x7F) == 0, 0x00, hi)
    nanb = (NAN_BYTE | sign).astype(np.uint8)
    return np.where(nan, nanb, lo).astype(np.uint8), np.where(nan, nanb, hi).astype(np.uint8)


def check_image(got8, b_bf16, scale, what):
    """Every byte of the [rows, cols] image `got8` inside its admissible pair, no allowed share of misses.  Returns the coverage
    of the case: {"two_byte": share of elements with two admissible non-zero-pair bytes, "saturated", "subnormal", "zero",
    "nan": counts, "n"}, all from the bf16 image."""
    got = _np(got8, np.uint8)
    b = _np(b_bf16, np.float32)
    assert got.ndim == 2 and got.shape == b.shape, (what, got.shape, b.shape)
    lo, hi = admissible(b, scale)
    kg, kl, kh = key(got), key(lo), key(hi)
    ref = quantize_ref(b, scale)
    mag = ref & 0x7F
    stats = {"n": int(got.size),
             "two_byte": float(((kh - kl) >= 1)[mag != 0].sum() + ((kh - kl) >= 2)[mag == 0].sum()) / got.size,
             "saturated": int((mag == 0x7E).sum()), "subnormal": int(((mag >= 1) & (mag <= SUB_MAX_BYTE)).sum()),
             "zero": int((mag == 0).sum()), "nan": int((mag == 0x7F).sum())}
    bad = (kg < kl) | (kg > kh)
    if not bad.any():
        return stats
    rows, cols = np.nonzero(bad)
    r0, c0 = int(rows[0]), int(cols[0])
    want = f"0x{lo[r0, c0]:02X}" if lo[r0, c0] == hi[r0, c0] else f"0x{lo[r0, c0]:02X}..0x{hi[r0, c0]:02X}"
    chunks = sorted(set(zip(rows.tolist(), (cols // 16).tolist())))
    bad_rows = sorted(set(rows.tolist()))
    # a displacement, not a rounding: the wrong bytes of a chunk are the expected bytes of another chunk of the same row, or a
    # wrong row holds another row's expected bytes
    moved = 0
    for r, ch in chunks[:64]:
        g = got[r, 16 * ch:16 * ch + 16]
        for o in range(0, got.shape[1], 16):
            if o != 16 * ch and g.size == ref[r, o:o + 16].size and (key(g) >= kl[r, o:o + 16]).all() and (key(g) <= kh[r, o:o + 16]).all():
                moved += 1
                break
    copied = 0
    for r in bad_rows[:16]:
        ok = ((kg[r][None, :] >= kl) & (kg[r][None, :] <= kh)).all(axis=1)
        ok[r] = False
        copied += bool(ok.any())
    elsewhere = sum(bool((ref[r] == got[r, c]).any()) for r, c in zip(rows[:256].tolist(), cols[:256].tolist()))
    nan_bytes = int(((got & 0x7F) == 0x7F)[bad].sum())
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {got.size} e4m3 bytes outside their admissible pair; first at (row {r0}, col {c0}): got "
        f"0x{got[r0, c0]:02X}, want {want} (bf16 value {float(b[r0, c0])!r}, scale {scale}); {len(chunks)} 16-byte chunks in "
        f"{len(bad_rows)} rows affected (rows {bad_rows[:8]}{'...' if len(bad_rows) > 8 else ''}); "
        f"{elsewhere} of the first {min(256, rows.size)} bad bytes occur among the expected bytes of their own row; "
        f"displacement: {moved} of the first {min(64, len(chunks))} bad chunks hold the expected bytes of another chunk of their row, "
        f"{copied} of the first {min(16, len(bad_rows))} bad rows hold another row's expected bytes; {nan_bytes} bad bytes are NaN bytes")
