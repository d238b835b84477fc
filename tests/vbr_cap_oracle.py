"""The rate cap of closed-loop variable-rate encoding (bvc_bvrnn_encode_vbr_capped) restated on top of vbr_oracle.py: the token bucket
as Python integers, the capped call in float32 and float64, the builder of the capped test cases, the window guarantee, and a numpy
statement of the wire of a streaming tick.  Shared by test_vbr_stream_cpu.py, test_gpu_vbr_cap.py and test_gpu_vbr_stream.py; the
references are computed once per case and nobody changes them.

Units are q8 (1/256 bit).  Per row and frame, once k_target - vbr_oracle.choose - is known:
  1. tok = min(burst_q8, tok + rate_q8)     2. a = the largest k with ladder[k] * 256 <= tok, 0 if there is none
  3. k* = min(k_target, a)                  4. tok = max(0, tok - ladder[k*] * 256)
and the frame goes on with k*.  If ladder[0] * 256 <= rate_q8, every window of L frames of a row holds 256 sum(bits) <= burst_q8 + L rate_q8."""
import functools

import numpy as np
import torch

import bvrnn_draws as bd
import vbr_oracle as vo
from oracle import bvrnn as obv

Q8 = 256


def bucket_step(tok, k_target, ladder, rate_q8, burst_q8):
    """One frame of one row: (k*, tok behind the frame, dict(a, clamped, floored)).  Integers only."""
    filled = int(tok) + int(rate_q8)
    tok = min(int(burst_q8), filled)
    a = max([k for k in range(len(ladder)) if int(ladder[k]) * Q8 <= tok], default=0)
    k = min(int(k_target), a)
    left = tok - int(ladder[k]) * Q8
    return k, max(0, left), dict(a=a, clamped=filled > int(burst_q8), floored=left < 0)


@torch.no_grad()
def _run(sd, y, ladder, target_fn, h0, dtype, cap, tok0):
    """vbr_oracle._run with the bucket between the choice and what the frame does with it.  cap: (rate_q8, burst_q8) or None."""
    sd = obv.cast_state(sd, dtype)
    y = torch.as_tensor(y).to(dtype)
    h = torch.as_tensor(h0).to(dtype)
    mean, std = sd["mean_mel"], sd["std_mel"]
    yn = (y - mean[None, None, :]) / std[None, None, :]
    px = obv.phi_x(sd, yn)
    zdim = sd["enc.4.weight"].shape[0]
    pos = torch.arange(zdim, dtype=dtype)[None, :]
    rungs = torch.tensor([float(n) for n in ladder], dtype=dtype)
    names = ("codes", "bits", "choice", "all_h", "prob", "dist", "dec", "tau", "k_target", "afford", "clamped", "floored")
    out = {n: [] for n in names}
    B = y.shape[0]
    rows = torch.arange(B)
    tok = None
    if cap is not None:
        tok = [int(cap[1])] * B if tok0 is None else [int(v) for v in tok0]
    for t in range(y.shape[1]):
        p = torch.sigmoid(obv.enc_logits(sd, torch.cat([px[:, t], h], 1)))
        z = torch.round(p)
        zk, pzk, dk = [], [], []
        for n in ladder:
            mask = (float(n) > pos).to(dtype)
            zz = z * mask + 0.5 * (1 - mask)
            pz = obv.phi_z(sd, zz)
            zk.append(zz); pzk.append(pz); dk.append(obv.dec(sd, torch.cat([pz, h], 1)))
        D = torch.stack([(d - y[:, t]).abs().mean(-1) for d in dk], 1)
        tau = target_fn(t, D, p).to(dtype)
        kt = vo.choose(D, tau)
        k = kt.clone()
        info = [dict(a=len(ladder) - 1, clamped=False, floored=False) for _ in range(B)]
        if cap is not None:
            for b in range(B):
                kb, tok[b], info[b] = bucket_step(tok[b], int(kt[b]), ladder, cap[0], cap[1])
                k[b] = kb
        zsel, pz, d = torch.stack(zk)[k, rows], torch.stack(pzk)[k, rows], torch.stack(dk)[k, rows]
        col = lambda key, dt: torch.tensor([i[key] for i in info], dtype=dt)[:, None]
        for name, v in (("codes", zsel), ("bits", rungs[k][:, None]), ("choice", k[:, None]), ("all_h", h), ("prob", p), ("dist", D), ("dec", d),
                        ("tau", tau[:, None]), ("k_target", kt[:, None]), ("afford", col("a", torch.long)),
                        ("clamped", col("clamped", torch.bool)), ("floored", col("floored", torch.bool))):
            out[name].append(v)
        pxg = obv.phi_x(sd, (d - mean[None, :]) / std[None, :])
        h = obv.gru_cell(sd, torch.cat([pxg, pz], 1), h)
    res = {k: torch.stack(v).permute(1, 0, 2).contiguous() for k, v in out.items()}
    for name in ("bits", "choice", "tau", "k_target", "afford", "clamped", "floored"):
        res[name] = res[name][:, :, 0]
    res["h_last"] = h
    res["tok_next"] = None if tok is None else torch.tensor(tok, dtype=torch.int64)
    return res


def encode_vbr_capped(sd, y, ladder, target, h0, rate_q8=None, burst_q8=None, tok0=None, dtype=torch.float32):
    """vbr_oracle.encode_vbr under the cap (rate_q8 None: without it, and then equal to it): its dict plus k_target, afford, clamped,
    floored (B,T) and tok_next (B,) int64 (None without a cap)."""
    target = torch.as_tensor(target)
    cap = None if rate_q8 is None else (int(rate_q8), int(burst_q8))
    return _run(sd, y, ladder, lambda t, D, p: target[:, t], h0, dtype, cap, tok0)


def make_case(h_dim, draw, B, T, ladder, rate_bits, burst_bits, margin=vo.MARGIN, seed=5):
    """vbr_oracle.make_case under a bucket of rate_bits per frame and burst_bits: the targets are written frame by frame as the capped
    float64 oracle goes, by that builder's rotation, a margin from every D_k the rule looks at (the rungs <= k_target)."""
    return _make_case(h_dim, draw, B, T, tuple(ladder), int(round(rate_bits * Q8)), int(round(burst_bits * Q8)), margin, seed)


@functools.lru_cache(maxsize=None)
def _make_case(h_dim, draw, B, T, ladder, rate_q8, burst_q8, margin, seed):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = bd.state_dict(h_dim, draw)
    y, _ = bd.inputs(B, T, seed=seed)
    h0 = torch.from_numpy((0.3 * np.random.default_rng(seed + 1).standard_normal((B, h_dim))).astype(np.float32))
    K = len(ladder)
    turn = [0] * K
    fallback = torch.zeros(B, T, dtype=torch.bool)

    def target_fn(t, D, p):
        tau = torch.empty(B, dtype=torch.float64)
        for b in range(B):
            d = D[b].tolist()
            if (t * B + b) % vo.FALLBACK_EVERY == vo.FALLBACK_EVERY - 1:
                tau[b] = min(d) - 2 * margin
                fallback[b, t] = True
                continue
            can = [0] + [k for k in range(1, K) if d[k] < min(d[:k]) - 2 * margin]
            k = min(can, key=lambda j: (turn[j], -j))
            turn[k] += 1
            tau[b] = d[0] + 2 * margin if k == 0 else 0.5 * (d[k] + min(d[:k]))
        return tau.float().double()

    o64 = _run(sd, y, ladder, target_fn, h0, torch.float64, (rate_q8, burst_q8), None)
    tau = o64["tau"].float()
    o32 = encode_vbr_capped(sd, y, ladder, tau, h0, rate_q8, burst_q8, dtype=torch.float32)
    looked = torch.arange(K)[None, None, :] <= torch.where(fallback, K - 1, o64["k_target"])[:, :, None]
    return vo.Case(sd=sd, y=y, h0=h0, ladder=ladder, tau=tau, o64=o64, o32=o32, fallback=fallback, looked=looked, h_dim=h_dim, draw=draw,
                   rate_q8=rate_q8, burst_q8=burst_q8)


def check_case(c, margin=vo.MARGIN):
    """What a capped case must show on the oracle alone before anything is compared with it."""
    o64, o32 = c.o64, c.o32
    gap = (o64["dist"] - c.tau.double()[:, :, None]).abs()
    assert float(gap[c.looked].min()) >= margin, float(gap[c.looked].min())
    binds = o64["afford"] < o64["k_target"]
    n_bind, n_free, n_clamp = int(binds.sum()), int((~binds).sum()), int(o64["clamped"].sum())
    assert n_bind >= 2 and n_free >= 2 and n_clamp >= 1, (n_bind, n_free, n_clamp)
    assert bool((o64["choice"] == torch.minimum(o64["k_target"], o64["afford"])).all())
    active = torch.arange(o64["prob"].shape[2]) < c.ladder[-1]
    tie = float((o64["prob"][:, :, active] - 0.5).abs().min())
    assert tie >= vo.TIE_P, tie
    assert torch.equal(o32["choice"], o64["choice"]) and torch.equal(o32["k_target"], o64["k_target"])
    assert torch.equal(o32["codes"].double(), o64["codes"]) and torch.equal(o32["tok_next"], o64["tok_next"])
    return n_bind, n_free, n_clamp


def check_windows(bits, rate_q8, burst_q8):
    """The guarantee, for every window of every row of bits (B,T): 256 sum(bits) <= burst_q8 + L rate_q8.  Returns the tightest slack."""
    b = np.rint(np.asarray(bits, dtype=np.float64)).astype(np.int64) * Q8
    T = b.shape[1]
    cs = np.concatenate([np.zeros((b.shape[0], 1), dtype=np.int64), np.cumsum(b, 1)], 1)
    slack = None
    for i in range(T):
        for j in range(i + 1, T + 1):
            s = int(burst_q8) + (j - i) * int(rate_q8) - (cs[:, j] - cs[:, i])
            assert (s >= 0).all(), (i, j, s.tolist())
            slack = int(s.min()) if slack is None else min(slack, int(s.min()))
    return slack


# ---------------------------------------------------------------------------------------------- the wire of a streaming tick, in numpy
def tick_wire(codes, bits, kmax):
    """codes (B,k,Z), bits (B,k) of one tick -> (packet buffer uint8 (B * kmax * stride,), sizes int32 (B,kmax)): frame j of row b at
    (b * kmax + j) * stride with stride = 1 + ceil(Z / 8), in the layout of vbr_oracle.pack_vbr; what the tick does not write is zero."""
    codes, bits = np.asarray(codes), np.asarray(bits)
    B, k, Z = codes.shape
    stride = vo.stride_of(Z)
    packed, sz = vo.pack_vbr(codes, bits)
    buf = np.zeros((B, kmax, stride), dtype=np.uint8)
    sizes = np.zeros((B, kmax), dtype=np.int32)
    buf[:, :k] = packed
    sizes[:, :k] = sz
    return buf.reshape(-1), sizes
