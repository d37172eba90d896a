"""Inputs of the Canny tests (tests/test_canny.py on the model, tests/test_canny_gpu.py on the kernels): images that reach every branch of
the non-maximum suppression, and state maps that are hard for a labelling scheme.  Everything is seeded numpy; no test changes them."""
import numpy as np

TW, TH = 64, 16                     # the kernels' tile (csrc/canny.hip: CN_TW, CN_TH)

CONTENTS = ("blur", "quant", "stairs", "checker", "noise")


def image(kind: str, H: int, W: int, C: int, seed: int = 0) -> np.ndarray:
    """uint8 [H, W, C].  blur: 5x5 box-blurred uniform noise (some ten weak pixels per strong one at 100 / 200); quant: the same in
    16 levels (ties); stairs: constant blocks of 3 x 5 pixels rising along both axes (every horizontal / vertical tie); checker: 0 / 255 blocks
    of 2 x 3 pixels in the left half and 0 / 255 diagonal stripes in the right one (mag = 1530, the largest a 3x3 Sobel pair can give); noise: raw uniform noise (every pixel strong)."""
    rng = np.random.default_rng(1000 * seed + 17 * H + 31 * W + C + 7 * CONTENTS.index(kind))
    if kind in ("blur", "quant"):
        n = rng.integers(0, 256, size=(H + 4, W + 4, C)).astype(np.int64)
        a = sum(n[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)) // 25
        if kind == "quant":
            a = a // 16 * 17
        return a.astype(np.uint8)
    if kind == "stairs":
        yy, xx = np.mgrid[0:H, 0:W]
        base = (yy // 3) * 37 + (xx // 5) * 53
        return np.stack([(base + 29 * c) % 256 for c in range(C)], axis=2).astype(np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.where(xx < (W + 1) // 2, ((yy // 2) + (xx // 3)) % 2, ((yy + xx) // 4) % 2).astype(np.uint8) * 255
        return np.stack([a] * C, axis=2) if C == 1 else np.stack([a, a, np.roll(a, 1, axis=1)], axis=2)
    if kind == "noise":
        return rng.integers(0, 256, size=(H, W, C)).astype(np.uint8)
    raise ValueError(kind)


# (1,1) .. (3,5); tile height +- 1 by tile width +- 1; two tiles + 1 in each direction
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)] + [(2 * TH + 1, 2 * TW + 1)]
SIZES_C3_ALIGN = [(5, 5), (5, 6), (5, 7)]           # 3 W mod 4 takes 3, 2, 1 (and 0 at W = 64)


# ---------------------------------------------------------------------------------------------- state maps
def random_map(H: int, W: int, density: float, strong: float = 0.01, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed + 1000 * H + W)
    cand = rng.random((H, W)) < density
    s = cand.astype(np.uint8)
    s[cand & (rng.random((H, W)) < strong)] = 2
    return s


def serpentine(H: int, W: int, strong: bool = True) -> np.ndarray:
    """A one-pixel path: every even row in full, odd rows one pixel at alternating ends; the strong pixel at the far end."""
    s = np.zeros((H, W), dtype=np.uint8)
    s[0::2, :] = 1
    for y in range(1, H, 2):
        s[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    if strong:
        last = H - 1 if (H - 1) % 2 == 0 else H - 2
        end_right = (last // 2) % 2 == 0            # row `last` is walked left to right when it is entered from the left
        s[last, W - 1 if end_right else 0] = 2
    return s


def spiral(H: int, W: int) -> np.ndarray:
    """A one-pixel rectangular spiral from the corner inwards with a one-pixel gap between its turns; the strong pixel at its inner end."""
    s = np.zeros((H, W), dtype=np.uint8)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W

    def free(y, x, dy, dx):                          # the next cell is empty and so is the one behind it
        return inside(y + dy, x + dx) and s[y + dy, x + dx] == 0 and not (inside(y + 2 * dy, x + 2 * dx) and s[y + 2 * dy, x + 2 * dx])

    y, x, dy, dx = 0, 0, 0, 1
    s[0, 0] = 1
    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy                        # turn right
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        s[y, x] = 1
    s[y, x] = 2
    return s


def diagonal(H: int, W: int) -> np.ndarray:
    """The main diagonal shifted so that it steps from (TH - 1, TW - 1) to (TH, TW): through a tile corner, connected by corners alone."""
    s = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        x = y + TW - TH
        if 0 <= x < W:
            s[y, x] = 1
    ys, xs = np.nonzero(s)
    s[ys[-1], xs[-1]] = 2
    return s


def two_components(H: int, W: int) -> np.ndarray:
    """Two blobs a one-pixel gap apart (column TW is empty), across a tile border; only the left one holds a strong pixel."""
    s = np.ones((H, W), dtype=np.uint8)
    s[:, TW] = 0
    s[0, 0] = 2
    return s


def all_weak_one_strong(H: int, W: int) -> np.ndarray:
    s = np.ones((H, W), dtype=np.uint8)
    s[H - 1, W // 2] = 2
    return s


def state_maps() -> dict:
    """name -> uint8 [H, W] map: what the hysteresis is tested on, by the model against scipy's labelling and by the kernels against the model."""
    H, W = 2 * TH + 1, 2 * TW + 1
    maps = {f"random {d} {h}x{w}": random_map(h, w, d) for d in (0.3, 0.41, 0.6) for h, w in ((70, 131), (H, W))}
    maps.update({
        "serpentine": serpentine(33, 67), "serpentine, no strong pixel": serpentine(33, 67, strong=False),
        "spiral": spiral(H, W), "diagonal": diagonal(H, W), "two components": two_components(H, W),
        "all weak, one strong": all_weak_one_strong(H, W), "all strong": np.full((H, W), 2, dtype=np.uint8),
        "all zero": np.zeros((H, W), dtype=np.uint8), "1 x N": random_map(1, 3 * TW + 5, 0.8, strong=0.05),
        "N x 1": random_map(3 * TH + 5, 1, 0.8, strong=0.05),
    })
    return maps
