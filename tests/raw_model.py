"""NumPy model of the raw-sensor gray conversion (what cv_bridge::toCvShare(msg, MONO8) computes for 16-bit and Bayer encodings), written from
the arithmetic the C header states and NOT from r-vio_amd/csrc/raw.h: whole-array slices of a padded image and one mask per site kind, no
per-pixel walk, no clamped coordinates.  The new raw tests (CPU and GPU) share it as their truth; everything is int64, every comparison exact."""
import numpy as np

KR, KG, KB = 4899, 9617, 1868
# where the red site of a pattern lies in the top-left 2 x 2 block, as (x, y); blue lies diagonally opposite
RED_AT = {"rggb": (0, 0), "bggr": (1, 1), "gbrg": (0, 1), "grbg": (1, 0)}
PATTERNS = ("rggb", "bggr", "gbrg", "grbg")          # in the order of the format values' low two bits
ROW_SWAP = {"rggb": "gbrg", "gbrg": "rggb", "bggr": "grbg", "grbg": "bggr"}
COL_SWAP = {"rggb": "grbg", "grbg": "rggb", "bggr": "gbrg", "gbrg": "bggr"}


def depth8(v):
    return (np.asarray(v, np.int64) + 128) // 257


def gray_px(r, g, b):
    return (np.asarray(r, np.int64) * KR + np.asarray(g, np.int64) * KG + np.asarray(b, np.int64) * KB + 8192) >> 14


def gray16(img, is_rgb=True):
    """H x W (mono16) or H x W x 3|4 uint16 -> H x W uint8"""
    img = np.asarray(img)
    if img.ndim == 2:
        return depth8(img).astype(np.uint8)
    r, b = (img[..., 0], img[..., 2]) if is_rgb else (img[..., 2], img[..., 0])
    return depth8(gray_px(r, img[..., 1], b)).astype(np.uint8)


def bayer_gray(img, pattern):
    """H x W mosaic (uint8 or uint16) -> H x W uint8"""
    img = np.asarray(img)
    h, w = img.shape
    assert h >= 3 and w >= 3
    p = np.pad(img.astype(np.int64), 1)                  # (what lies outside only reaches the border outputs, which are overwritten below)
    c = p[1:-1, 1:-1]
    ns, ew = p[:-2, 1:-1] + p[2:, 1:-1], p[1:-1, :-2] + p[1:-1, 2:]
    dg = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    rx, ry = RED_AT[pattern]
    yy, xx = np.mgrid[0:h, 0:w]
    red_col, red_row = (xx % 2) == rx, (yy % 2) == ry
    y = np.zeros((h, w), np.int64)
    at_red, at_blue = red_col & red_row, ~red_col & ~red_row
    g_in_red_row, g_in_blue_row = ~red_col & red_row, red_col & ~red_row
    y[at_red] = ((4 * KR * c + KG * (ns + ew) + KB * dg + 32768) >> 16)[at_red]
    y[at_blue] = ((4 * KB * c + KG * (ns + ew) + KR * dg + 32768) >> 16)[at_blue]
    y[g_in_red_row] = ((2 * KG * c + KR * ew + KB * ns + 16384) >> 15)[g_in_red_row]
    y[g_in_blue_row] = ((2 * KG * c + KB * ew + KR * ns + 16384) >> 15)[g_in_blue_row]
    y[:, 0], y[:, -1] = y[:, 1], y[:, -2]               # columns first,
    y[0], y[-1] = y[1], y[-2]                           # then rows
    if img.dtype == np.uint16:
        y = depth8(y)
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


def mosaic(rgb, pattern):
    """sample an H x W x 3 (R, G, B) image through the pattern's colour filter array -> H x W of the same dtype"""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    rx, ry = RED_AT[pattern]
    yy, xx = np.mgrid[0:h, 0:w]
    red_col, red_row = (xx % 2) == rx, (yy % 2) == ry
    out = rgb[..., 1].copy()
    out[red_col & red_row] = rgb[..., 0][red_col & red_row]
    out[~red_col & ~red_row] = rgb[..., 2][~red_col & ~red_row]
    return out


def to_gray(img, encoding):
    """the converted 8-bit image of any encoding name the library takes (mono8 ... bayer_grbg16)"""
    img = np.asarray(img)
    if encoding.startswith("bayer_"):
        return bayer_gray(img, encoding[6:10])
    if encoding == "mono8":
        return img.astype(np.uint8)
    if encoding.endswith("16"):
        return gray16(img, encoding.startswith("rgb"))
    r, b = (img[..., 0], img[..., 2]) if encoding.startswith("rgb") else (img[..., 2], img[..., 0])
    return gray_px(r, img[..., 1], b).astype(np.uint8)
