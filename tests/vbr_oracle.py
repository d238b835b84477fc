"""Closed-loop variable-rate encoding (bvc_bvrnn_encode_vbr) restated with the functions of oracle/bvrnn.py, the builder of the test
cases whose targets keep every decision a margin away from a tie, and a numpy statement of the per-frame wire format.  Shared by
test_vbr_cpu.py and test_gpu_vbr.py; the references are computed once per case and nobody changes them.

Per row b and frame t at state h_t:  p = sigmoid(enc([phi_x(norm(y_t)), h_t])), z = round(p);  for every rung k of the ladder
z^k = z on positions < n_k and 0.5 behind them, d^k = dec([phi_z(z^k), h_t]), D_k = mean_j |d^k_j - y_tj|;  k* = the first k with
D_k <= tau[b, t], the last rung if there is none;  codes = z^{k*}, bits = n_{k*}, h_{t+1} = GRU([phi_x(norm(d^{k*})), phi_z(z^{k*})], h_t)."""
import functools

import numpy as np
import torch

import bvrnn_draws as bd
from oracle import bvrnn as obv

MARGIN = 1e-4             # every D the rule looks at lies at least this far from its target
TIE_P = 5e-6              # every probability that can reach a candidate lies at least this far from 0.5
FALLBACK_EVERY = 5        # every fifth frame of a case has a target below every D


def choose(D, tau):
    """(B, K) distortions, (B,) targets -> (B,) long: the first rung with D_k <= tau, the last one if there is none (NaN compares false)."""
    ok = D <= tau[:, None]
    K = D.shape[1]
    first = torch.where(ok, torch.arange(K)[None, :], torch.full_like(ok, K, dtype=torch.long)).min(dim=1).values
    return torch.where(first < K, first, torch.full_like(first, K - 1))


@torch.no_grad()
def _run(sd, y, ladder, target_fn, h0, dtype):
    """target_fn(t, D (B,K), p (B,Z)) -> tau (B,) in `dtype`."""
    sd = obv.cast_state(sd, dtype)
    y = torch.as_tensor(y).to(dtype)
    h = torch.as_tensor(h0).to(dtype)
    mean, std = sd["mean_mel"], sd["std_mel"]
    yn = (y - mean[None, None, :]) / std[None, None, :]
    px = obv.phi_x(sd, yn)
    zdim = sd["enc.4.weight"].shape[0]
    pos = torch.arange(zdim, dtype=dtype)[None, :]
    rungs = torch.tensor([float(n) for n in ladder], dtype=dtype)
    out = dict(codes=[], bits=[], choice=[], all_h=[], prob=[], dist=[], dec=[], tau=[])
    B = y.shape[0]
    rows = torch.arange(B)
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
        k = choose(D, tau)
        zsel, pz, d = torch.stack(zk)[k, rows], torch.stack(pzk)[k, rows], torch.stack(dk)[k, rows]
        for name, v in (("codes", zsel), ("bits", rungs[k][:, None]), ("choice", k[:, None]), ("all_h", h), ("prob", p), ("dist", D), ("dec", d),
                        ("tau", tau[:, None])):
            out[name].append(v)
        pxg = obv.phi_x(sd, (d - mean[None, :]) / std[None, :])
        h = obv.gru_cell(sd, torch.cat([pxg, pz], 1), h)
    res = {k: torch.stack(v).permute(1, 0, 2).contiguous() for k, v in out.items()}
    for name in ("bits", "choice", "tau"):
        res[name] = res[name][:, :, 0]
    res["h_last"] = h
    return res


def encode_vbr(sd, y, ladder, target, h0, dtype=torch.float32):
    """y (B,T,80), ladder ascending bit counts, target (B,T), h0 (B,H) -> dict(codes (B,T,Z), bits (B,T), choice (B,T) long, all_h
    (B,T,H) [the state BEFORE frame t], prob (B,T,Z), dist (B,T,K), dec (B,T,80), h_last (B,H))."""
    target = torch.as_tensor(target)
    return _run(sd, y, ladder, lambda t, D, p: target[:, t], h0, dtype)


class Case(dict):
    __getattr__ = dict.__getitem__


def make_case(h_dim, draw, B, T, ladder, margin=MARGIN, seed=5):
    """The float64 oracle on inputs(B, T, seed) of the draw's checkpoint, with the targets written frame by frame as it goes: among the
    rungs that CAN be "the first with D_k <= tau" - rung 0, and every k with D_k < min(D_0 .. D_{k-1}) - 2 margin - one is picked in
    rotation (the one picked least often so far) and tau put halfway between D_k and that minimum (rung 0: 2 margin above D_0); every FALLBACK_EVERY-th frame tau lies
    2 margin below every D, so that no rung meets it.  Returns a Case: sd, y, h0, ladder, tau (B,T) float32, o64 / o32 (encode_vbr of
    the two precisions on that tau), fallback (B,T) bool, looked (B,T,K) bool - the rungs the rule looks at."""
    return _make_case(h_dim, draw, B, T, tuple(ladder), margin, seed)


@functools.lru_cache(maxsize=None)
def _make_case(h_dim, draw, B, T, ladder, margin, seed):
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
            if (t * B + b) % FALLBACK_EVERY == FALLBACK_EVERY - 1:
                tau[b] = min(d) - 2 * margin
                fallback[b, t] = True
                continue
            can = [0] + [k for k in range(1, K) if d[k] < min(d[:k]) - 2 * margin]
            k = min(can, key=lambda j: (turn[j], -j))      # in rotation: the rung picked least often so far, the higher one of equals
            turn[k] += 1
            tau[b] = d[0] + 2 * margin if k == 0 else 0.5 * (d[k] + min(d[:k]))
        return tau.float().double()              # the targets are float32 numbers: both precisions and the GPU see the same ones

    o64 = _run(sd, y, ladder, target_fn, h0, torch.float64)
    tau = o64["tau"].float()
    o32 = encode_vbr(sd, y, ladder, tau, h0, torch.float32)
    looked = torch.arange(K)[None, None, :] <= torch.where(fallback, K - 1, o64["choice"])[:, :, None]
    return Case(sd=sd, y=y, h0=h0, ladder=ladder, tau=tau, o64=o64, o32=o32, fallback=fallback, looked=looked, h_dim=h_dim, draw=draw)


def check_case(c, margin=MARGIN):
    """What a case must show on the oracle alone before anything is compared with it."""
    K = len(c.ladder)
    o64, o32 = c.o64, c.o32
    gap = (o64["dist"] - c.tau.double()[:, :, None]).abs()
    assert float(gap[c.looked].min()) >= margin, float(gap[c.looked].min())
    chosen = o64["choice"][~c.fallback]
    counts = [int((chosen == k).sum()) for k in range(K)]
    assert all(n >= 2 for n in counts) and int(c.fallback.sum()) >= 2, (counts, int(c.fallback.sum()))
    assert bool((o64["choice"][c.fallback] == K - 1).all())
    active = torch.arange(o64["prob"].shape[2]) < c.ladder[-1]
    tie = float((o64["prob"][:, :, active] - 0.5).abs().min())
    assert tie >= TIE_P, tie
    assert torch.equal(o32["choice"], o64["choice"]) and torch.equal(o32["codes"].double(), o64["codes"])
    return counts


# ---------------------------------------------------------------------------------------------- the wire format, in numpy
def stride_of(z_dim):
    return 1 + (z_dim + 7) // 8


def pack_vbr(codes, bits):
    """codes (B,T,Z) float with 1.0 where a bit is set, bits (B,T) -> (bytes uint8 (B,T,1 + ceil(Z/8)), sizes int32 (B,T)): byte 0 the
    frame's bit count n, then ceil(n/8) bytes with bit i at byte i/8, LSB first, then zeros; sizes = 1 + ceil(n/8)."""
    codes, bits = np.asarray(codes), np.asarray(bits)
    B, T, Z = codes.shape
    out = np.zeros((B, T, stride_of(Z)), dtype=np.uint8)
    sizes = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        for t in range(T):
            n = int(min(max(bits[b, t], 0), Z))
            out[b, t, 0] = n
            for i in range(n):
                if codes[b, t, i] > 0.75:
                    out[b, t, 1 + i // 8] |= 1 << (i % 8)
            sizes[b, t] = 1 + (n + 7) // 8
    return out, sizes


def unpack_vbr(packed, z_dim):
    """Inverse: a header above z_dim reads as z_dim; positions >= n are 0.5."""
    packed = np.asarray(packed)
    B, T, S = packed.shape
    assert S == stride_of(z_dim)
    codes = np.full((B, T, z_dim), 0.5, dtype=np.float32)
    bits = np.zeros((B, T), dtype=np.float32)
    for b in range(B):
        for t in range(T):
            n = min(int(packed[b, t, 0]), z_dim)
            bits[b, t] = n
            for i in range(n):
                codes[b, t, i] = (packed[b, t, 1 + i // 8] >> (i % 8)) & 1
    return codes, bits
