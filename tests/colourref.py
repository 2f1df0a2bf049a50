"""The normative colour conversion in numpy (include/streamoptima.h, "Colour conversion"): 8-bit
RGB <-> this codec's padded 4:2:0 planes, int32 with 16 fractional bits, `>>` an arithmetic shift.
The GPU kernels (so_colour.hip) must equal this bit for bit; test_colour.py checks it against the
float64 formulas."""
import numpy as np

K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def float_forward(matrix: str, full_range: bool) -> np.ndarray:
    """The real-valued forward matrix (rows Y, Cb, Cr; columns R, G, B), range scaling included."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    return np.array([[ys * kr, ys * kg, ys * kb],
                     [-cs * kr / (2 * (1 - kb)), -cs * kg / (2 * (1 - kb)), cs * 0.5],
                     [cs * 0.5, -cs * kg / (2 * (1 - kr)), -cs * kb / (2 * (1 - kr))]], np.float64)


def float_inverse(matrix: str, full_range: bool) -> np.ndarray:
    """The inverse of float_forward in closed form (rows R, G, B; columns Y - yoff, U - 128, V - 128)."""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    yi, ci = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return np.array([[yi, 0.0, ci * 2 * (1 - kr)],
                     [yi, -ci * 2 * kb * (1 - kb) / kg, -ci * 2 * kr * (1 - kr) / kg],
                     [yi, ci * 2 * (1 - kb), 0.0]], np.float64)


def forward_table(matrix: str, full_range: bool) -> np.ndarray:
    """F = rint(coef * 65536), the G entry of each row then adjusted so that the Y row sums to
    rint(ys * 65536) and the chroma rows to 0."""
    f = np.rint(float_forward(matrix, full_range) * 65536.0).astype(np.int64)
    ys = 1.0 if full_range else 219.0 / 255.0
    want = (int(np.rint(ys * 65536.0)), 0, 0)
    for r in range(3):
        f[r, 1] += want[r] - int(f[r].sum())
    return f.astype(np.int32)


def inverse_table(matrix: str, full_range: bool) -> np.ndarray:
    """J = rint(M * 65536), no adjustment."""
    return np.rint(float_inverse(matrix, full_range) * 65536.0).astype(np.int32)


def yoff(full_range: bool) -> int:
    return 0 if full_range else 16


def rgb_to_yuv420(rgb: np.ndarray, matrix: str, full_range: bool, hp: int, wp: int):
    """rgb: uint8 [F, h, w, 3] (h, w even) -> (y [F, hp, wp], uv [F, 2, hp/2, wp/2]) uint8, every
    sample outside the picture area 128."""
    rgb = np.asarray(rgb)
    n, h, w, _ = rgb.shape
    assert h % 2 == 0 and w % 2 == 0 and hp % 2 == 0 and wp % 2 == 0 and hp >= h and wp >= w
    f = forward_table(matrix, full_range).astype(np.int32)
    p = rgb.astype(np.int32)
    y = np.full((n, hp, wp), 128, np.uint8)
    uv = np.full((n, 2, hp // 2, wp // 2), 128, np.uint8)
    acc = f[0, 0] * p[..., 0] + f[0, 1] * p[..., 1] + f[0, 2] * p[..., 2] + np.int32((yoff(full_range) << 16) + 32768)
    y[:, :h, :w] = np.clip(acc >> 16, 0, 255)
    s = p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]     # [F, h/2, w/2, 3]
    for c in (1, 2):
        acc = f[c, 0] * s[..., 0] + f[c, 1] * s[..., 1] + f[c, 2] * s[..., 2] + np.int32((128 << 18) + (1 << 17))
        uv[:, c - 1, :h // 2, :w // 2] = np.clip(acc >> 18, 0, 255)
    return y, uv


def yuv420_to_rgb(y: np.ndarray, uv: np.ndarray, h: int, w: int, matrix: str, full_range: bool) -> np.ndarray:
    """Padded planes y [F, hp, wp], uv [F, 2, hp/2, wp/2] -> uint8 [F, h, w, 3]; each chroma
    sample serves its 2 x 2 luma samples."""
    j = inverse_table(matrix, full_range).astype(np.int32)
    yy = np.asarray(y)[:, :h, :w].astype(np.int32) - yoff(full_range)
    c = np.asarray(uv)[:, :, :h // 2, :w // 2].astype(np.int32) - 128
    c = np.repeat(np.repeat(c, 2, axis=2), 2, axis=3)
    out = np.empty(yy.shape + (3,), np.uint8)
    for k in range(3):
        acc = j[k, 0] * yy + j[k, 1] * c[:, 0] + j[k, 2] * c[:, 1] + np.int32(32768)
        out[..., k] = np.clip(acc >> 16, 0, 255)
    return out


PRIMARIES = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)


def sample_frames(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """uint8 [n, h, w, 3]: random content, the 8 saturated primaries as 2 x 2 cells along the top
    rows where they fit (else as single pixels)."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for k, c in enumerate(PRIMARIES):
        if 2 * k + 2 <= w:
            rgb[:, 0:2, 2 * k:2 * k + 2] = c
        else:
            rgb[:, (k // w) % h, k % w] = c
    return rgb
