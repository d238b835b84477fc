"""The rate cap of closed-loop variable-rate encoding on the GPU (bvc_bvrnn_encode_vbr_capped): the select kernel alone on pinned
distortions, targets and buckets, the whole capped call against the float64 oracle on cases where the cap binds (vbr_cap_oracle), a
bucket that never binds against the uncapped entry bit for bit, batch / chunk invariance with the buckets carried across the cut, and
the library's refusals.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import vbr_cap_oracle as vc
import vbr_oracle as vo
from bvcodec import _abi
from gpu_common import DEV, make_model

pytestmark = pytest.mark.gpu

X = 80
BVC_EINVAL = -1
CASES = ((128, "wide", 5, 20, (8, 16, 32, 64), 20, 96), (1024, "default", 3, 6, (17, 35, 64), 30, 70))
LADDERS = {1: (24,), 3: (0, 17, 64), 8: (1, 2, 4, 8, 16, 32, 48, 64)}


def model_of(h_dim, draw, var_bit=True):
    return make_model(var_bit, h_dim, seed=bd.seed_of(h_dim, draw), gains=bd.GAINS[draw])[0]


# ---------------------------------------------------------------------------------------------- 1: the select kernel alone
def run_select_capped(mel, y, tau, ladder, rate_q8, burst_q8, tok):
    lib = _abi.load()
    K, B, _ = mel.shape
    md, yd, td = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (mel, y, tau))
    D = torch.full((B, K), float("nan"), device=DEV)
    choice = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    bits = torch.full((B,), float("nan"), device=DEV)
    tk = torch.tensor(tok, dtype=torch.int32, device=DEV)
    lad = (ctypes.c_int32 * K)(*ladder)
    with torch.cuda.device(DEV):
        _abi.check(lib.bvc_test_vbr_select_capped(_abi.ptr(md), _abi.ptr(yd), _abi.ptr(td), lad, K, B, X, _abi.ptr(D),
                                                  ctypes.c_void_p(choice.data_ptr()), _abi.ptr(bits), _abi.current_stream(torch.device(DEV)),
                                                  rate_q8, burst_q8, ctypes.c_void_p(tk.data_ptr())))
    torch.cuda.synchronize()
    return D.cpu().numpy(), choice.cpu().numpy(), bits.cpu().numpy(), tk.cpu().numpy()


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("B", [5, 17])
def test_select_capped_exact(B, K):
    """Exact distortions as in test_gpu_vbr.test_select_exact (small integers times 2^-3), D_k falling with k; targets that ask for
    every rung, and buckets pinned at the edges of step 2: exactly a rung's price once the rate is added, one q8 short of it, empty,
    full, above the burst (step 1 clamps).  The choice, the bits and the bucket behind the frame are the integers of bucket_step."""
    lad = LADDERS[K]
    rng = np.random.default_rng(300 * B + K)
    y = rng.integers(-64, 64, size=(B, X)).astype(np.float32) / 8
    m = rng.integers(1, 4, size=(B, X))
    sign = rng.choice([-1, 1], size=(K, B, X))
    mel = y[None] + sign * (K - np.arange(K))[:, None, None] * m[None] / 8.0
    D_ref = (((K - np.arange(K))[None, :] * m.sum(1)[:, None]).astype(np.float32) / np.float32(8)) / np.float32(X)
    rate_q8, burst_q8 = 777, 40 * 256
    tau = np.empty(B, dtype=np.float32)
    tok, k_target = [], []
    for b in range(B):
        kt = (b * 3 + 1) % K
        tau[b] = D_ref[b, kt] if b % 5 else -np.inf                  # D_k == tau picks rung k; -inf: the top rung, a rate target
        kt = kt if b % 5 else K - 1
        k_target.append(kt)
        price = lad[(b + 2) % K] * 256
        tok.append(max(0, (price - rate_q8, price - rate_q8 - 1, 0, burst_q8, burst_q8 - 5, price)[b % 6]))
    D, choice, bits, tok_out = run_select_capped(mel, y, tau, lad, rate_q8, burst_q8, tok)
    assert np.array_equal(D, D_ref)
    want = [vc.bucket_step(tok[b], k_target[b], lad, rate_q8, burst_q8) for b in range(B)]
    assert choice.tolist() == [w[0] for w in want], (choice, want)
    assert tok_out.tolist() == [w[1] for w in want]
    assert np.array_equal(bits, np.array(lad, dtype=np.float32)[choice])
    if K > 1:                                                         # what the pins are there for
        assert any(w[2]["a"] < kt for w, kt in zip(want, k_target)) and any(w[2]["a"] >= kt for w, kt in zip(want, k_target))
        assert any(w[2]["clamped"] for w in want)


def test_select_capped_floor_of_step_4():
    """A rate below rung 0: nothing is affordable, rung 0 goes out and the bucket stops at zero."""
    lad = (8, 16)
    y = np.zeros((3, X), np.float32)
    mel = np.stack([y + 1.0, y + 0.5])
    tau = np.full(3, -np.inf, np.float32)
    _, choice, bits, tok = run_select_capped(mel, y, tau, lad, 2 * 256, 8 * 256, [0, 5 * 256, 8 * 256])
    assert choice.tolist() == [0, 0, 0] and bits.tolist() == [8.0, 8.0, 8.0] and tok.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- 2: the whole call against float64
def run_case(c, model, rows=None, frames=None, h=None, tok=None, cap=True):
    rows = slice(None) if rows is None else rows
    frames = slice(None) if frames is None else frames
    y = c.y[rows, frames].contiguous().to(DEV)
    t = c.tau[rows, frames].contiguous().to(DEV)
    h0 = (c.h0[rows] if h is None else h).reshape(1, -1, c.h_dim).to(DEV)
    kw = dict(rate_q8=c.rate_q8, burst_q8=c.burst_q8, tok=tok) if cap else {}
    codes, bits, all_h, extra = model.bvrnn.encode_vbr(y, c.ladder, t, h0, return_all=True, **kw)
    torch.cuda.synchronize()
    return dict(codes=codes.cpu(), bits=bits.cpu(), all_h=all_h.cpu(), **{k: v.cpu() for k, v in extra.items()})


_RUNS = {}


def case_run(case):
    if case not in _RUNS:
        c = vc.make_case(*case)
        vc.check_case(c)
        _RUNS[case] = (c, run_case(c, model_of(case[0], case[1])))
    return _RUNS[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"h{c[0]}-{c[1]}")
def test_capped_call_against_float64(case):
    """Choices, bits, codes and the buckets equal; D, the states and the decoded mel within test_gpu_vbr.py's bars."""
    c, got = case_run(case)
    o64, o32 = c.o64, c.o32
    rungs = torch.tensor(c.ladder, dtype=torch.float64)
    assert torch.equal(got["bits"].double(), o64["bits"]), (got["bits"], o64["bits"])
    assert torch.equal(got["bits"].double(), rungs[o64["choice"]])
    assert torch.equal(got["codes"].double(), o64["codes"])
    assert got["tok_next"].dtype == torch.int32 and torch.equal(got["tok_next"].long(), o64["tok_next"])
    v = bd.compare(bd.n64(got["dist"]), bd.n64(o64["dist"]), bd.n64(o32["dist"]), f"dist {case}")
    e_h = float((got["all_h"].double() - o64["all_h"]).abs().max())
    e_hn = float((got["h_next"][0].double() - o64["h_last"]).abs().max())
    e_d = float((got["dec"].double() - o64["dec"]).abs().max())
    print(f"  dist ratio {v.ratio:.3f} e_hip {v.e_hip:.3e} e32 {v.e32:.3e}; all_h {e_h:.3e} h_next {e_hn:.3e} dec {e_d:.3e}")
    assert v.ok, v.message
    assert e_h <= 2e-5 and e_hn <= 2e-5, (e_h, e_hn)
    assert e_d <= 2e-4, e_d
    vc.check_windows(got["bits"].numpy(), c.rate_q8, c.burst_q8)      # the guarantee, on the GPU's own bits


# ---------------------------------------------------------------------------------------------- 3: a cap that is off
def test_cap_that_never_binds_is_the_uncapped_entry():
    """A bucket refilled to the top rung before every frame changes no choice: every output equals the uncapped entry's bit for bit,
    and the uncapped entry gives what it gave (test_gpu_vbr.py checks it against the uncapped oracle)."""
    case = CASES[0]
    c = vc.make_case(*case)
    model = model_of(case[0], case[1])
    plain = run_case(c, model, cap=False)
    top = c.ladder[-1] * 256
    y, t, h0 = c.y.to(DEV), c.tau.to(DEV), c.h0[None].to(DEV)
    codes, bits, all_h, extra = model.bvrnn.encode_vbr(y, c.ladder, t, h0, return_all=True, rate_q8=top, burst_q8=top)
    torch.cuda.synchronize()
    assert "tok_next" not in plain
    assert torch.equal(codes.cpu(), plain["codes"]) and torch.equal(bits.cpu(), plain["bits"]) and torch.equal(all_h.cpu(), plain["all_h"])
    for k in ("prob", "dist", "dec", "h_next"):
        assert torch.equal(extra[k].cpu(), plain[k]), k
    assert torch.equal(extra["tok_next"].cpu().long(), ((c.ladder[-1] - plain["bits"][:, -1]) * 256).long())
    assert not torch.equal(plain["bits"].double(), c.o64["bits"])                 # (the case's own cap does change the result)


# ---------------------------------------------------------------------------------------------- 4: batch and chunk invariance
def test_rows_and_chunks_are_invariant_with_tok_carried():
    case = CASES[0]
    c, whole = case_run(case)
    model = model_of(case[0], case[1])
    names = ("codes", "bits", "all_h", "dist", "dec", "prob")
    for b in range(c.y.shape[0]):
        one = run_case(c, model, rows=slice(b, b + 1))
        for k in names:
            assert torch.equal(one[k], whole[k][b:b + 1]), (k, b)
        assert torch.equal(one["tok_next"], whole["tok_next"][b:b + 1])
    for cut in (1, 10, 13):                                           # the cut wherever: the state and the buckets travel
        a = run_case(c, model, frames=slice(0, cut))
        z = run_case(c, model, frames=slice(cut, 20), h=a["h_next"], tok=a["tok_next"])
        for k in names:
            assert torch.equal(torch.cat([a[k], z[k]], 1), whole[k]), (k, cut)
        assert torch.equal(z["h_next"], whole["h_next"]) and torch.equal(z["tok_next"], whole["tok_next"])
    # the facade: a waveform under the cap equals the coder's capped call on the facade's mel, zero state, full buckets
    big = model_of(1024, "default")
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 256 * 30)).astype(np.float32) * 0.1).to(DEV)
    codes, bits = big.encode_vbr(x, -float("inf"), bitrates=(1500, 3000, 6000), rate_cap=2600, burst=96)
    from bvcodec.model import cap_q8
    rate_q8, burst_q8 = cap_q8(big.conf, [17, 35, 64], 2600, 96)
    c2, b2, _ = big.bvrnn.encode_vbr(big.mel_spectrogram(x), (17, 35, 64), -float("inf"), torch.zeros(1, 3, 1024, device=DEV),
                                     rate_q8=rate_q8, burst_q8=burst_q8)
    assert torch.equal(c2, codes) and torch.equal(b2, bits)
    vc.check_windows(bits.cpu().numpy(), rate_q8, burst_q8)
    assert len(set(bits[0].tolist())) >= 2                            # a rate target: the bucket decides, and not always alike


# ---------------------------------------------------------------------------------------------- 5: refusals from the library
def raw_call(model, rate_q8, burst_q8, B=2, T=4, ladder=(16, 32)):
    eng = model.engine()
    lib = eng.lib
    Z = model.conf["z_dim"]
    K = len(ladder)
    y, tau = torch.zeros(B, T, X, device=DEV), torch.zeros(B, T, device=DEV)
    codes, bits = torch.empty(B, T, Z, device=DEV), torch.empty(B, T, device=DEV)
    need = lib.bvc_vbr_workspace_bytes(eng.handle, B, T, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lad = (ctypes.c_int32 * K)(*ladder)
    with torch.cuda.device(DEV):
        rc = lib.bvc_bvrnn_encode_vbr_capped(eng.handle, _abi.ptr(y), _abi.ptr(tau), lad, K, None, B, T, _abi.ptr(codes), _abi.ptr(bits), None,
                                             None, None, None, None, ctypes.c_void_p(ws.data_ptr()), need, eng.stream(), rate_q8, burst_q8,
                                             None, None)
    torch.cuda.synchronize()
    return rc, lib.bvc_last_error().decode()


def test_library_refusals():
    var = model_of(128, "wide")
    assert raw_call(var, 0, 16 * 256)[0] == 0                         # NULL buckets in and out: full, dropped
    for rate, burst in ((-1, 16 * 256), (5, -1)):
        rc, msg = raw_call(var, rate, burst)
        assert rc == BVC_EINVAL and "negative" in msg, (rc, msg)
    rc, msg = raw_call(var, 5, 16 * 256 - 1)
    assert rc == BVC_EINVAL and "never holds rung 0" in msg, (rc, msg)
    rc, msg = raw_call(var, 5, 16 * 256, ladder=(32, 16))
    assert rc == BVC_EINVAL and "rung" in msg, (rc, msg)
    assert raw_call(var, 0, 16 * 256)[0] == 0                         # and the model is as usable as before
