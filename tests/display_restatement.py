"""The display transform restated in numpy from the text of DESIGN.md 2.20 (it shares no code with the library): every operation on float32
arrays, one numpy operation -- one rounding -- per operator, in the order the text writes them.  The encode counts thresholds with a sorted
search, not with the library's eight-step one.  The tables are arguments: the tests hand it the library's, so that a last-bit difference
between two pow implementations cannot look like a pixel bug; tables() below is the f64 computation the library's are compared with."""
import math

import numpy as np

F = np.float32
CLAMP, REINHARD, FILMIC = 0, 1, 2
SRGB, GAMMA22, REFERENCE = 0, 1, 2
BINS = 2048


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def thresholds(encode):
    """T[0] = 0 and T[1..255] in f64."""
    k = np.arange(1, 256, dtype=np.float64)
    v = (k - 0.5) / 255.0
    if encode == SRGB:
        lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    else:
        lin = v ** 2.2
    return np.concatenate([[0.0], lin])


def gamma_table():
    return np.array([min(max(math.floor(math.pow(i / 255.0, 1.0 / 2.2) * 255.0), 0), 255) for i in range(256)], np.uint8)


def lum(c):
    return (F(0.212671) * c[..., 0] + F(0.715160) * c[..., 1]) + F(0.072169) * c[..., 2]


def valid(rgb):
    return np.isfinite(rgb).all(axis=2)


def floored(rgb):
    with np.errstate(invalid="ignore"):
        return np.where(rgb < 0, F(0), rgb).astype(np.float32)


def histogram(rgb):
    """The 2048 counts: valid pixels whose luminance is a normal finite number, by bits >> 20."""
    rgb = np.asarray(rgb, np.float32)
    with np.errstate(all="ignore"):
        bits = np.ascontiguousarray(lum(floored(rgb))).view(np.uint32)
    counted = valid(rgb) & (bits >= 0x00800000) & (bits < 0x7f800000)
    return np.bincount(bits[counted] >> 20, minlength=BINS).astype(np.uint32)


def pick(hist, permille, key):
    """The f32 scale: key over the centre of the first bin whose running count exceeds the rank; 1 when nothing was counted."""
    n = int(hist.astype(np.uint64).sum())
    if n == 0:
        return F(1.0)
    rank = (n - 1) * int(permille) // 1000
    b = int(np.searchsorted(np.cumsum(hist.astype(np.uint64)), rank, side="right"))
    centre = np.array([(b << 20) | (1 << 19)], np.uint32).view(np.float32)[0]
    with np.errstate(all="ignore"):
        return F(key) / centre


def curve_of(c, curve, inv_white2):
    """c [h, w, 3] f32, already scaled."""
    one = F(1.0)
    with np.errstate(all="ignore"):
        if curve == REINHARD:
            y = lum(c)
            yd = (y * (one + y * F(inv_white2))) / (one + y)
            m = yd / y
            out = c * m[..., None]
            out[y == 0] = 0
            return out
        if curve == FILMIC:
            return (c * (F(2.51) * c + F(0.03))) / (c * (F(2.43) * c + F(0.59)) + F(0.14))
    return c


def encode_of(x, encode, table):
    """x [h, w, 3] f32 -> codes [h, w, 3] uint8.  table: f32 [256] thresholds (T[0] unused), or uint8 [256] for the reference encode."""
    x = np.where(np.isnan(x), F(np.inf), x).astype(np.float32)
    if encode == REFERENCE:
        with np.errstate(all="ignore"):
            q = np.clip(np.floor(x.astype(np.float64) * 255.0), 0.0, 255.0).astype(np.int64)
        return np.asarray(table, np.uint8)[q]
    t = np.asarray(table, np.float32)[1:]
    return np.searchsorted(t, x.reshape(-1), side="right").reshape(x.shape).astype(np.uint8)


def display(rgb, curve, encode, table, auto, permille=500, exposure=1.0, key=0.18, inv_white2=0.0, invalid_rgba=0xff000000):
    """rgb [h, w, 3] f32 -> (rgba8 [h, w, 4], the f32 scale used)."""
    rgb = np.asarray(rgb, np.float32)
    scale = pick(histogram(rgb), permille, key) if auto else F(exposure)
    with np.errstate(all="ignore"):
        c = floored(rgb) * scale
    codes = encode_of(curve_of(c, curve, inv_white2), encode, table)
    out = np.empty(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = codes
    out[..., 3] = 255
    out[~valid(rgb)] = [(invalid_rgba >> s) & 0xff for s in (0, 8, 16, 24)]
    return out, scale
