"""LPIPS v0.1 (net='alex') written out from its definition, for the tests: a float64 torch-CPU statement that does not
import irm_amd.perceptual, the same chain in float32 (its distance from the float64 one sizes the tolerance of the GPU
path), synthetic parameters, test frames, and the numpy statement of the space-to-depth frame irm_lpips_pack writes.

Definition: x = code / peak (the value itself for float32), v = 2 x - 1, u_c = (v_c - shift_c) / scale_c; AlexNet's
`features` tapped after each ReLU; per tap d_l = mean_{y,x} sum_c lin[c] (f_c / (n_f + 1e-10) - g_c / (n_g + 1e-10))^2
with n_f = sqrt(sum_c f_c^2); LPIPS = sum_l d_l."""
import numpy as np
import torch
import torch.nn.functional as F

from irm_amd import synth

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10
#: (key prefix, C_out, C_in, kernel, stride, pad, max-pool 3 s2 first)
LAYERS = (("features.0", 64, 3, 11, 4, 2, False), ("features.3", 192, 64, 5, 1, 2, True),
          ("features.6", 384, 192, 3, 1, 1, True), ("features.8", 256, 384, 3, 1, 1, False),
          ("features.10", 256, 256, 3, 1, 1, False))
ALEX_SHAPES = {}
for _p, _co, _ci, _k, _s, _pad, _pool in LAYERS:
    ALEX_SHAPES[_p + ".weight"] = (_co, _ci, _k, _k)
    ALEX_SHAPES[_p + ".bias"] = (_co,)
LIN_SHAPES = {f"lin{l}.model.1.weight": (1, t[1], 1, 1) for l, t in enumerate(LAYERS)}
PEAK = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0, np.dtype(np.float32): 1.0}
DTYPES = (np.uint8, np.uint16, np.float32)


def synth_states(seed=7):
    """(alex_state, lin_state): synthetic AlexNet weights and lin vectors, lin the absolute value of a synthetic tensor."""
    alex = synth.synth_state_dict(ALEX_SHAPES, seed=seed)
    lin = {k: v.abs() for k, v in synth.synth_state_dict(LIN_SHAPES, seed=seed + 1).items()}
    return alex, lin


def scaled(img, dtype=torch.float64):
    """u [1, 3, H, W] of an HWC frame."""
    x = torch.from_numpy(np.ascontiguousarray(img).astype(np.float64)).to(dtype) / PEAK[img.dtype]
    v = 2 * x - 1
    u = (v - torch.tensor(SHIFT, dtype=dtype)) / torch.tensor(SCALE, dtype=dtype)
    return u.permute(2, 0, 1)[None]


def features(img, alex, dtype=torch.float64):
    t, taps = scaled(img, dtype), []
    for p, _, _, _, stride, pad, pool in LAYERS:
        if pool:
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, alex[p + ".weight"].to(dtype), alex[p + ".bias"].to(dtype), stride=stride, padding=pad))
        taps.append(t[0])
    return taps


def head(f, g, lin):
    """d_l of maps f, g [C, H, W] and lin [C], in the maps' dtype."""
    lin = lin.reshape(-1, 1, 1).to(f.dtype)
    nf = (f * f).sum(0, keepdim=True).sqrt()
    ng = (g * g).sum(0, keepdim=True).sqrt()
    d = f / (nf + EPS) - g / (ng + EPS)
    return float((lin * d * d).sum(0).mean())


def lpips(pred, target, alex, lin, dtype=torch.float64):
    """(the five d_l, their sum) of two HWC numpy frames."""
    fp, ft = features(pred, alex, dtype), features(target, alex, dtype)
    taps = [head(f, g, lin[f"lin{l}.model.1.weight"]) for l, (f, g) in enumerate(zip(fp, ft))]
    return taps, float(sum(taps))


def random_frame(h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return rng.random((h, w, 3)).astype(np.float32)
    return rng.integers(0, int(PEAK[np.dtype(dtype)]) + 1, (h, w, 3)).astype(dtype)


def as_dtype(img_u8, dtype):
    """A uint8 frame in another frame dtype with the same x = code / peak (uint16: code x 257)."""
    if dtype == np.uint8:
        return img_u8
    if dtype == np.uint16:
        return img_u8.astype(np.uint16) * 257
    return (img_u8.astype(np.float64) / 255).astype(np.float32)


def pairs(h, w, dtype, seed=0):
    """name -> (pred, target): a random pair, a frame against its blurred copy, a frame against itself, a black frame
    against a random one."""
    blurred, sharp = synth.synth_image_pair(seed, h, w, 3, blur=7)
    a, b = random_frame(h, w, dtype, 100 + seed), random_frame(h, w, dtype, 200 + seed)
    return {"random": (a, b), "blurred": (as_dtype(blurred, dtype), as_dtype(sharp, dtype)), "same": (a, a.copy()),
            "black": (np.zeros_like(a), b)}


def affine(dtype):
    """(a, b) float32 [3]: u_c = raw a_c + b_c, made in float64 and rounded once."""
    peak = PEAK[np.dtype(dtype)]
    a = np.array([2.0 / (peak * s) for s in SCALE], np.float64).astype(np.float32)
    b = np.array([(-1.0 - m) / s for m, s in zip(SHIFT, SCALE)], np.float64).astype(np.float32)
    return a, b


def out_size(n):
    return (n - 7) // 4 + 1


def space_to_depth(u):
    """u [3, H, W] float64 -> z [48, OH + 2, OW + 2]: z[c 16 + i 4 + j][Y][X] = u[c][4 Y + i - 2][4 X + j - 2], 0 outside
    rows 0 .. min(H, 4 OH + 5) - 1 (columns alike)."""
    _, h, w = u.shape
    oh, ow = out_size(h), out_size(w)
    hr, wr = min(h, 4 * oh + 5), min(w, 4 * ow + 5)
    big = np.zeros((3, 4 * (oh + 2), 4 * (ow + 2)), np.float64)
    big[:, 2:2 + hr, 2:2 + wr] = u[:, :hr, :wr]
    z = big.reshape(3, oh + 2, 4, ow + 2, 4).transpose(0, 2, 4, 1, 3)
    return np.ascontiguousarray(z).reshape(48, oh + 2, ow + 2)


def pack_model(img):
    """The float64 evaluation of raw a_c + b_c with the float32 a, b the device uses, space-to-depth."""
    a, b = affine(img.dtype)
    u = img.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)
    return space_to_depth(u.transpose(2, 0, 1))
