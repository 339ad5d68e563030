"""The selective scan of the MaIR path: seeded inputs in three parameter regimes, the device launch on planar inputs, a
float64 restatement of the recurrence, and the check that holds a device result to it with the fp32 oracle
(oracle/mair_ref.py) as yardstick.  Used by tests/test_gpu_mair.py, tests/test_gpu_guard_bands.py and
tests/test_gpu_degenerate_ops.py."""
import numpy as np
import torch
import torch.nn.functional as F

from irm_amd import ops, synth
from oracle import mair_ref

#: float64 bar of the scan / combine tests: e_dev <= SCAN_K * e_32 + SCAN_F * max|y64|, e_32 the fp32 oracle's own error
SCAN_K = 4.0
SCAN_F = 2.0 ** -22


def rnd(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(321, name, shape, lo, hi)


def scan_lanes(D):
    """Channels a float64 check covers: the first and last lane of every 64-channel block, and all of a partial block."""
    ch = set()
    for db in range(-(-D // 64)):
        lo, hi = 64 * db, min(64 * db + 64, D)
        ch.update(range(lo, hi) if hi - lo < 64 else (lo, hi - 1))
    return torch.tensor(sorted(ch))


def selective_scan_f64(u, dt_raw, dtb, A, Bs, Cs, Ds):
    """Float64 restatement of the recurrence, vectorised over (batch, direction, channel, state), looped over time,
    y formed on the fly (no [L]-long state history).  u, dt_raw (B, 4, d, L) in scan order; dtb, Ds (4, d);
    A (4, d, N); Bs, Cs (B, 4, N, L).  dt = softplus(dt_raw + dtb); h_t = exp(dt A) h + dt B_t u_t;
    y_t = <h_t, C_t> + Ds u_t."""
    u, A, Bs, Cs = u.double(), A.double(), Bs.double(), Cs.double()
    dt = F.softplus(dt_raw.double() + dtb.double().unsqueeze(-1))
    h = torch.zeros(u.shape[:3] + (A.shape[-1],), dtype=torch.float64)
    y = torch.empty(u.shape, dtype=torch.float64)
    for t in range(u.shape[-1]):
        d_t = dt[..., t].unsqueeze(-1)
        h = torch.exp(d_t * A) * h + (d_t * u[..., t].unsqueeze(-1)) * Bs[:, :, None, :, t]
        y[..., t] = (h * Cs[:, :, None, :, t]).sum(-1)
    return y + Ds.double().unsqueeze(-1) * u


def scan_inputs(tag, regime, B, D, N, R, L):
    """(x planar u (B, D, L), proj [dt_raw | B | C] per direction in pixel order (B, 4, J, L), dtw, dtb, A, Ds).
    synthetic: dt bias in [-4, -2], A in [-4.5, -1] (the original op test);
    trained: A = -(1..N) as Mamba initialises it, dt bias = softplus^-1(dt), dt log-uniform in [1e-3, 1e-1];
    memory: dt ~ 1e-3 and |A| <= 1 (a chunk keeps most of its incoming state), with raw dt spikes beyond -20 and +20 on
    1 % of the steps so both softplus tails run."""
    J = R + 2 * N
    x = rnd(f"su{tag}", (B, D, L))
    proj = rnd(f"sp{tag}", (B, 4, J, L))
    Ds = rnd(f"sd{tag}", (4 * D,), 0.5, 1.5)
    if regime == "synthetic":
        dtw = rnd(f"sw{tag}", (4, D, R), -0.5, 0.5)
        dtb = rnd(f"sb{tag}", (4, D), -4, -2)
        A = -torch.exp(rnd(f"sa{tag}", (4 * D, N), 0, 1.5))
    elif regime == "trained":
        dtw = rnd(f"sw{tag}", (4, D, R), -0.1, 0.1)
        dt = torch.exp(rnd(f"sb{tag}", (4, D), float(np.log(1e-3)), float(np.log(1e-1))).double())
        dtb = torch.log(torch.expm1(dt)).float()
        A = -torch.arange(1, N + 1, dtype=torch.float32).repeat(4 * D, 1)
    else:
        dtw = rnd(f"sw{tag}", (4, D, R), 0.5, 1.5) / R
        dtb = torch.full((4, D), float(np.log(np.expm1(1e-3))))
        A = -rnd(f"sa{tag}", (4 * D, N), 0.05, 1.0)
        spike = rnd(f"sx{tag}", (B, 4, 1, L), 0, 1)
        amp = torch.where(rnd(f"sy{tag}", (B, 4, 1, L)) > 0, 40.0, -40.0)
        proj[:, :, :R] = torch.where(spike < 0.01, amp, proj[:, :, :R] * 0.5)
    return x, proj, dtw, dtb, A, Ds


def run_scan(dev, x, proj, dtw, dtb, A, Ds, ids, B, L, D, N, R, chunk):
    """The device scan on planar inputs: (y (B, 4, L, D) in pixel order, ysum (B, 4, DB, nchunk, 64), nchunk)."""
    J = R + 2 * N
    xT = x.transpose(1, 2).contiguous().to(dev)                                             # (B,L,D)
    pT = proj.reshape(B, 4 * J, L).transpose(1, 2).contiguous().to(dev)                     # (B,L,4J)
    nchunk, DB = -(-L // chunk), -(-D // 64)
    yT = torch.full((B, 4, L, D), float("nan"), device=dev)
    state = torch.empty(2 * B * 4 * DB * nchunk * N * 64, device=dev)
    sdt = torch.empty(B * 4 * DB * nchunk * 64, device=dev)
    ysum = torch.empty(B * 4 * DB * nchunk * 64, device=dev)
    ops.selective_scan(xT, pT, ids.int().to(dev), dtw.to(dev), dtb.to(dev), A.to(dev), Ds.to(dev), yT, state, sdt, ysum,
                       B, L, D, N, R, chunk)
    return yT, ysum.view(B, 4, DB, nchunk, 64), nchunk


def ysum_floor(chunk, nchunk, mabs):
    """Worst-case rounding of the device's chunk sums of y divided by L (sequential fp32 sums of `chunk` steps, then
    16 interleaved partial sums over the chunks), given mabs = max over channels of mean|y|: inherent to an fp32 sum,
    about 1e-5 relative at chunk 176 - a chunk missing from the sum moves the mean by 1 / nchunk."""
    return (chunk + nchunk // 16 + 16) * 2.0 ** -24 * mabs


def check_scan_f64(tag, x, proj, dtw, dtb, A, Ds, ids, inv, got, ysum, B, L, D, N, R, chunk):
    """got (B, 4, D, L) pixel order, ysum (B, 4, DB, nchunk, 64) from the device, against the float64 restatement on
    the scan_lanes(D) channels; yardstick: the fp32 oracle (mair_ref.selective_scan) on the same channels."""
    ch = scan_lanes(D)
    d = len(ch)
    xs = torch.stack([x[:, ch].index_select(-1, ids[k]) for k in range(4)], 1)              # (B,4,d,L) scan order
    pg = torch.stack([proj[:, k].index_select(-1, ids[k]) for k in range(4)], 1)            # (B,4,J,L)
    w_c, b_c, A_c, D_c = dtw[:, ch], dtb[:, ch], A.view(4, D, N)[:, ch], Ds.view(4, D)[:, ch]
    y64 = selective_scan_f64(xs, torch.einsum("bkrl,kdr->bkdl", pg[:, :, :R].double(), w_c.double()), b_c, A_c,
                             pg[:, :, R:R + N], pg[:, :, R + N:], D_c)
    dts = torch.einsum("bkrl,kdr->bkdl", pg[:, :, :R], w_c)
    y32 = mair_ref.selective_scan(xs.reshape(B, -1, L), dts.reshape(B, -1, L), A_c.reshape(-1, N), pg[:, :, R:R + N],
                                  pg[:, :, R + N:], D_c.reshape(-1), delta_bias=b_c.reshape(-1),
                                  delta_softplus=True).view(B, 4, d, L)
    y64 = torch.stack([y64[:, k].index_select(-1, inv[k]) for k in range(4)], 1)            # pixel order
    y32 = torch.stack([y32[:, k].index_select(-1, inv[k]) for k in range(4)], 1)
    g = got[:, :, ch].double()
    ymax = float(y64.abs().max())
    e_dev, e_32 = float((g - y64).abs().max()), float((y32.double() - y64).abs().max())
    m64 = y64.mean(-1)
    s = ysum.cpu().double().sum(3).reshape(B, 4, -1)[:, :, ch] / L
    m_dev, m_32 = float((s - m64).abs().max()), float((y32.double().mean(-1) - m64).abs().max())
    floor = ysum_floor(chunk, ysum.shape[3], float(y64.abs().mean(-1).max()))
    print(f"scan {tag}: y e_dev {e_dev:.3e} e_32 {e_32:.3e} ratio {e_dev / e_32:.2f} (|y64| {ymax:.3g}); "
          f"mean e_dev {m_dev:.3e} e_32 {m_32:.3e} fp32-sum floor {floor:.3e}")
    assert e_dev <= SCAN_K * e_32 + SCAN_F * ymax, "scan output vs float64"
    assert m_dev <= SCAN_K * m_32 + floor, "chunk-summed ysum / L vs float64 mean"
