"""Degenerate inputs, stated once: the pixels, images and frames on which a normalising kernel reaches the branches
that independent uniform noise never reaches (a zero mean square, a zero variance, a variance far below eps, the
sqrt(K - 1) bound of a normalised deviation).  Shared by tests/test_degenerate_cpu.py (which proves the properties
claimed here), tests/test_gpu_degenerate_ops.py and tests/test_gpu_degenerate_models.py.

Pixel patterns over K channels.  Each is chosen so that the LayerNorm arithmetic is exact in fp32 whatever the
summation order (all partial sums are dyadic numbers of a few bits), so a kernel that misses a float64 reference on them
cannot blame conditioning:
  Z       all channels 0
  C(a)    all channels a, a in {1, -2, 0.5}: mean exactly a, variance exactly 0
  A(a)    a + 2^-12 on even channels, a - 2^-12 on odd ones: mean a, variance exactly 2^-24 (far below eps = 1e-5, from
          a flat pixel and not from a global amplitude)
  S       one-hot, channel 0 = 1: the normalised deviation of channel 0 reaches sqrt(K - 1), the bound behind
          _hip.ln_split_scale and _hip.gram_scales"""
import torch

from irm_amd import synth

C_VALUES = (1.0, -2.0, 0.5)
A_DELTA = 2.0 ** -12
A_VAR = 2.0 ** -24

#: label of each pattern in the `labels` map of patterned_image (0 = noise)
PATTERNS = {"Z": 1, "C(1)": 2, "C(-2)": 3, "C(0.5)": 4, "A(1)": 5, "A(-2)": 6, "A(0.5)": 7, "S": 8}
#: labels of the pixels whose LayerNorm output is exactly the bias under WithBias (zero deviation from the mean)
FLAT_LABELS = (1, 2, 3, 4)


def pattern(name, K, dtype=torch.float32):
    """The K channel values of a pattern by its name in PATTERNS."""
    if name == "Z":
        return torch.zeros(K, dtype=dtype)
    if name == "S":
        v = torch.zeros(K, dtype=dtype)
        v[0] = 1.0
        return v
    a = float(name[2:-1])
    if name[0] == "C":
        return torch.full((K,), a, dtype=dtype)
    sign = torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0).to(dtype)
    return a + A_DELTA * sign


def _labels_2d(H, W, th, tw):
    """Whole tiles first, single pixels on top: tile (1, 1) of Z, tile (1, 0) of C(1) (clipped at the image), then the
    first and last pixel and both sides of the first tile seam in each direction."""
    lab = torch.zeros(H, W, dtype=torch.long)
    lab[th:2 * th, tw:2 * tw] = PATTERNS["Z"]
    lab[th:2 * th, :tw] = PATTERNS["C(1)"]
    lab[0, 0] = PATTERNS["Z"]
    lab[H - 1, W - 1] = PATTERNS["S"]
    if tw < W:
        lab[0, tw - 1], lab[0, tw] = PATTERNS["C(-2)"], PATTERNS["A(1)"]
    if th < H:
        lab[th - 1, 0], lab[th, 0] = PATTERNS["C(0.5)"], PATTERNS["A(-2)"]
    return lab


def _labels_1d(N, t):
    """The same on the flattened pixel index, for kernels whose tile is a run of t pixels: pixel tiles 2 and 3 whole,
    the first and last pixel, both sides of the first tile seam."""
    lab = torch.zeros(N, dtype=torch.long)
    lab[2 * t:3 * t] = PATTERNS["Z"]
    lab[3 * t:4 * t] = PATTERNS["C(1)"]
    lab[0] = PATTERNS["Z"]
    if t < N:
        lab[t - 1], lab[t] = PATTERNS["C(-2)"], PATTERNS["A(1)"]
    if t + 1 < N:
        lab[t + 1] = PATTERNS["C(0.5)"]
    if t + 2 < N:
        lab[t + 2] = PATTERNS["A(0.5)"]
    lab[N - 1] = PATTERNS["S"]
    return lab


def patterned_image(tag, B, K, H, W, tile, lo=-1.5, hi=2.0, seed=977):
    """(x [B][K][H][W] float32, labels [H][W]): uniform noise in [lo, hi) with the patterns placed relative to `tile`,
    (rows, columns) for the 8 x 32 tiles of the fused branch kernels or a pixel count for the GEMMs' runs of 16 / 64
    pixels.  Every image of the batch carries the same labels over its own noise."""
    x = synth.uniform(seed, f"degenerate_{tag}", (B, K, H, W), lo, hi)
    lab = _labels_2d(H, W, *tile) if isinstance(tile, tuple) else _labels_1d(H * W, int(tile)).view(H, W)
    for name, code in PATTERNS.items():
        m = lab == code
        if bool(m.any()):
            x[:, :, m] = pattern(name, K).view(1, K, 1)
    return x, lab


def all_pattern_image(name, B, K, H, W):
    """Every pixel of every image the same pattern (all-Z: a black tile of a bias-free network; all-C(1): a flat one)."""
    return pattern(name, K).view(1, K, 1, 1).expand(B, K, H, W).contiguous()


def flat_mask(labels):
    """[H][W] bool: the Z and C(a) pixels."""
    m = torch.zeros_like(labels, dtype=torch.bool)
    for code in FLAT_LABELS:
        m |= labels == code
    return m


def flat_neighbourhood_mask(labels):
    """[H][W] bool: pixels whose 3 x 3 neighbourhood, as far as it lies inside the image, is wholly Z / C(a) (a
    zero-padded stencil sees nothing else there)."""
    f = flat_mask(labels).float()[None, None]
    bad = torch.nn.functional.max_pool2d(1.0 - f, 3, 1, 1)[0, 0]      # the padding value of max_pool2d is -inf
    return bad == 0.0


FRAMES = ("black", "low", "high", "flat_hot", "letterbox", "checker", "ramp")


def frame(kind, shape, lo, hi, seed=7):
    """A whole-model input [B][C][H][W] in the range (lo, hi) of a ledger case."""
    B, C, H, W = shape
    if kind == "black":
        return torch.zeros(shape)
    if kind == "low":
        return torch.full(shape, float(lo))
    if kind == "high":
        return torch.full(shape, float(hi))
    if kind == "flat_hot":
        x = torch.full(shape, 0.5 * (lo + hi))
        x[:, :, H // 2, W // 2] = hi
        return x
    if kind == "letterbox":
        x = synth.uniform(seed, f"degenerate_frame_{shape}", shape, lo, hi)
        x[:, :, :H // 4] = lo
        x[:, :, H - H // 4:] = lo
        return x
    if kind == "checker":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        return torch.where((yy + xx) % 2 == 0, float(lo), float(hi)).expand(shape).contiguous()
    if kind == "ramp":
        return torch.linspace(lo, hi, W).view(1, 1, 1, W).expand(shape).contiguous()
    raise ValueError(kind)
