"""Closed-loop variable-rate encoding on the GPU (bvc_bvrnn_encode_vbr): the select kernel alone on data whose distortions are exact,
the whole call against the float64 oracle on cases whose targets keep every decision a margin from a tie (vbr_oracle.make_case), one
rung against the plain encoder bit for bit, batch / chunk invariance, the receiver side with the per-frame wire format, and the
library's refusals.  Needs the MI355X: run with ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import bvrnn_draws as bd
import vbr_oracle as vo
from bvcodec import _abi
from gpu_common import DEV, make_model, on_schedule

pytestmark = pytest.mark.gpu

X = 80
BVC_EINVAL = -1
CASES = ((128, "wide", 5, 20, (8, 16, 32, 64)), (1024, "default", 3, 6, (17, 35, 64)))


def model_of(h_dim, draw, var_bit=True):
    return make_model(var_bit, h_dim, seed=bd.seed_of(h_dim, draw), gains=bd.GAINS[draw])[0]


# ---------------------------------------------------------------------------------------------- 1: the select kernel alone
def run_select(mel, y, tau, ladder):
    """mel (K,B,X), y (B,X), tau (B,) float32 -> D (B,K), choice (B,), bits (B,) as numpy."""
    lib = _abi.load()
    K, B, _ = mel.shape
    md, yd, td = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (mel, y, tau))
    D = torch.full((B, K), float("nan"), device=DEV)
    choice = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    bits = torch.full((B,), float("nan"), device=DEV)
    lad = (ctypes.c_int32 * K)(*ladder)
    with torch.cuda.device(DEV):
        _abi.check(lib.bvc_test_vbr_select(_abi.ptr(md), _abi.ptr(yd), _abi.ptr(td), lad, K, B, X, _abi.ptr(D),
                                           ctypes.c_void_p(choice.data_ptr()), _abi.ptr(bits), _abi.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    return D.cpu().numpy(), choice.cpu().numpy(), bits.cpu().numpy()


def rule(D, tau):
    """The first rung with D_k <= tau, the last if none: numpy, row by row."""
    out = []
    for d, t in zip(D, tau):
        ok = [k for k in range(len(d)) if d[k] <= t]
        out.append(ok[0] if ok else len(d) - 1)
    return np.array(out)


LADDERS = {1: (24,), 3: (0, 17, 64), 8: (1, 2, 4, 8, 16, 32, 48, 64)}


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("B", [5, 17])
def test_select_exact(B, K):
    """Differences that are small integers times 2^-3: every |d - y|, their sum and so D = sum / 80 are exact in float32 in any order.
    D_k falls with k, so a target EQUAL to D_k picks rung k; the other rows take a target between two rungs, one below every D (the
    fallback), NaN, +inf and -inf."""
    rng = np.random.default_rng(100 * B + K)
    y = rng.integers(-64, 64, size=(B, X)).astype(np.float32) / 8
    m = rng.integers(1, 4, size=(B, X))
    sign = rng.choice([-1, 1], size=(K, B, X))
    mel = y[None] + sign * (K - np.arange(K))[:, None, None] * m[None] / 8.0
    # (B, K): an integer, its eighth, and the one rounded operation, the division by 80
    D_ref = (((K - np.arange(K))[None, :] * m.sum(1)[:, None]).astype(np.float32) / np.float32(8)) / np.float32(X)
    tau = np.empty(B, dtype=np.float32)
    for b in range(B):
        kind = b % 6
        if kind == 0:
            tau[b] = D_ref[b, b % K]                              # D_k == tau: chosen
        elif kind == 1:
            tau[b] = D_ref[b].min() - 1.0                         # nothing meets it: the last rung
        elif kind == 2:
            tau[b] = np.nan
        elif kind == 3:
            tau[b] = np.inf
        elif kind == 4:
            tau[b] = -np.inf
        else:
            tau[b] = np.nextafter(D_ref[b, (b // 6) % K], np.float32(0))      # one ulp below D_k: rung k is NOT taken
    D, choice, bits = run_select(mel, y, tau, LADDERS[K])
    assert np.array_equal(D, D_ref), np.abs(D - D_ref).max()
    want = rule(D_ref, tau)
    assert np.array_equal(choice, want), (choice, want)
    assert np.array_equal(bits, np.array(LADDERS[K], dtype=np.float32)[want])
    for b in range(B):                                            # what the kinds are there for
        if b % 6 == 0:
            assert choice[b] == b % K
        if b % 6 in (1, 2, 4):
            assert choice[b] == K - 1
        if b % 6 == 3:
            assert choice[b] == 0


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("B", [5, 17])
def test_select_normal_data(B, K):
    """N(0, 1) data: |D - D64| <= 8 x max(e32, 2^-24 |D64|), e32 the CPU float32 mean's own distance (the project's bar)."""
    g = torch.Generator().manual_seed(7 * B + K)
    mel, y = torch.randn(K, B, X, generator=g), torch.randn(B, X, generator=g)
    D64 = (mel.double() - y.double()[None]).abs().mean(-1).T.contiguous()
    D32 = (mel - y[None]).abs().mean(-1).T.contiguous()
    tau = D64.median(dim=1).values.float()
    D, choice, bits = run_select(mel.numpy(), y.numpy(), tau.numpy(), LADDERS[K])
    v = bd.compare(D[None], D64.numpy()[None], D32.numpy()[None], f"select D B={B} K={K}")
    print(f"  select D: ratio {v.ratio:.3f} e_hip {v.e_hip:.3e} e32 {v.e32:.3e}")
    assert v.ok, v.message
    assert np.array_equal(choice, rule(D, tau.numpy()))           # the rule on the kernel's own D
    assert np.array_equal(bits, np.array(LADDERS[K], dtype=np.float32)[choice])


# ---------------------------------------------------------------------------------------------- 2: the whole call against float64
def run_case(c, model, rows=None, frames=None, h=None, ladder=None, tau=None):
    rows = slice(None) if rows is None else rows
    frames = slice(None) if frames is None else frames
    y = c.y[rows, frames].contiguous().to(DEV)
    t = (c.tau if tau is None else tau)[rows, frames].contiguous().to(DEV)
    h0 = (c.h0[rows] if h is None else h).reshape(1, -1, c.h_dim).to(DEV)
    codes, bits, all_h, extra = model.bvrnn.encode_vbr(y, c.ladder if ladder is None else ladder, t, h0, return_all=True)
    torch.cuda.synchronize()
    return dict(codes=codes.cpu(), bits=bits.cpu(), all_h=all_h.cpu(), **{k: v.cpu() for k, v in extra.items()})


_RUNS = {}


def case_run(case):
    """The case's float64 reference and the GPU's answer to it, computed once."""
    if case not in _RUNS:
        c = vo.make_case(*case)
        vo.check_case(c)
        _RUNS[case] = (c, run_case(c, model_of(case[0], case[1])))
    return _RUNS[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"h{c[0]}-{c[1]}")
def test_whole_call_against_float64(case):
    c, got = case_run(case)
    o64, o32 = c.o64, c.o32
    assert torch.equal(got["bits"].double(), o64["bits"]), (got["bits"], o64["bits"])
    assert torch.equal(got["codes"].double(), o64["codes"])
    v = bd.compare(bd.n64(got["dist"]), bd.n64(o64["dist"]), bd.n64(o32["dist"]), f"dist {case}")
    e_h = float((got["all_h"].double() - o64["all_h"]).abs().max())
    e_hn = float((got["h_next"][0].double() - o64["h_last"]).abs().max())
    e_d = float((got["dec"].double() - o64["dec"]).abs().max())
    e_p = float((got["prob"].double() - o64["prob"]).abs().max())
    print(f"  dist ratio {v.ratio:.3f} e_hip {v.e_hip:.3e} e32 {v.e32:.3e}; all_h {e_h:.3e} h_next {e_hn:.3e} dec {e_d:.3e} prob {e_p:.3e}")
    assert v.ok, v.message
    assert e_h <= 2e-5 and e_hn <= 2e-5, (e_h, e_hn)
    assert e_d <= 2e-4, e_d


# ---------------------------------------------------------------------------------------------- 3: one rung is the plain encoder
@pytest.mark.parametrize("schedule", ["layers", "default"])
@pytest.mark.parametrize("n", [16, 64])
def test_one_rung_equals_encode(n, schedule):
    c = vo.make_case(*CASES[0])
    model = model_of(128, "wide")
    eng = model.engine()
    y, h0 = c.y.to(DEV), c.h0[None].to(DEV)
    B, T = c.y.shape[:2]
    bits = torch.full((B, T), float(n), device=DEV)

    def plain():
        return model.bvrnn.encode(y, bits, h0)
    try:
        eng.set_option("encode_fold", 0)
        codes, all_h = on_schedule(model, "layers", plain) if schedule == "layers" else [t.clone() for t in plain()]
        vc, vb, vh = model.bvrnn.encode_vbr(y, (n,), torch.full((B, T), float("nan")), h0)
        torch.cuda.synchronize()
    finally:
        eng.set_option("encode_fold", 1)
    assert torch.equal(vc, codes) and torch.equal(vh, all_h)
    assert bool((vb == n).all())


# ---------------------------------------------------------------------------------------------- 4: batch and chunk invariance
def test_rows_and_chunks_are_invariant():
    case = CASES[0]
    c, whole = case_run(case)
    model = model_of(case[0], case[1])
    names = ("codes", "bits", "all_h", "dist", "dec", "prob")
    for b in range(c.y.shape[0]):                                   # every row alone
        one = run_case(c, model, rows=slice(b, b + 1))
        for k in names:
            assert torch.equal(one[k], whole[k][b:b + 1]), (k, b)
    a = run_case(c, model, frames=slice(0, 10))                     # 10 + 10 frames with the state carried
    z = run_case(c, model, frames=slice(10, 20), h=a["h_next"])
    for k in names:
        assert torch.equal(torch.cat([a[k], z[k]], 1), whole[k]), k
    assert torch.equal(z["h_next"], whole["h_next"])
    # another K and T in the same process, on the same workspace: the step graph is keyed by the rungs
    c2 = vo.make_case(case[0], case[1], 5, 7, (16, 64))
    vo.check_case(c2)
    two = run_case(c2, model)
    assert torch.equal(two["bits"].double(), c2.o64["bits"]) and torch.equal(two["codes"].double(), c2.o64["codes"])
    again = run_case(c, model)                                      # and back: the first graph is still good
    for k in names:
        assert torch.equal(again[k], whole[k]), k


# ---------------------------------------------------------------------------------------------- 5: the receiver side
def test_decoder_reconstructs_what_the_encoder_reported():
    c, got = case_run(CASES[0])
    model = model_of(128, "wide")
    mel, _ = model.bvrnn.decode(got["codes"].to(DEV), c.h0[None].to(DEV))
    e = float((mel.cpu() - got["dec"]).abs().max())
    print(f"  decode(codes) against the encoder's dec: {e:.3e}")
    assert e <= 2e-5, e                     # the encoder's and the decoder's order of summation differ (dec.0, the GRU's input gates)


def test_wire_format_round_trip_through_the_facade():
    model = model_of(1024, "default")
    Z = 64
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 256 * 12)).astype(np.float32) * 0.1).to(DEV)
    tau = torch.tensor([[0.0, np.inf, np.nan, -np.inf] * 3] * 2)            # last rung, rung 0, last, last
    codes, bits = model.encode_vbr(x, tau, bitrates=(1500, 3000, 6000))
    assert bits.tolist() == [[64.0, 17.0, 64.0, 64.0] * 3] * 2
    packed, sizes = model.pack_vbr(codes, bits)
    ref_packed, ref_sizes = vo.pack_vbr(codes.cpu().numpy(), bits.cpu().numpy())
    assert np.array_equal(packed.cpu().numpy(), ref_packed) and np.array_equal(sizes.cpu().numpy(), ref_sizes)
    assert torch.equal(sizes.cpu(), (1 + torch.ceil(bits.cpu() / 8)).to(torch.int32))
    back, nb = model.unpack_vbr(packed)
    assert torch.equal(back, codes) and torch.equal(nb, bits)
    n = x.shape[1]
    assert torch.equal(model.decode(back, n), model.decode(codes, n))
    # random bytes: a header of 255 unpacks as z_dim bits, and whatever the bytes hold the result is the numpy statement's
    wild = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(2, 12, 9)).astype(np.uint8))
    wild[0, 0, 0] = 255
    wc, wb = model.unpack_vbr(wild.to(DEV))
    rc, rb = vo.unpack_vbr(wild.numpy(), Z)
    assert wb[0, 0] == Z and np.array_equal(wc.cpu().numpy(), rc) and np.array_equal(wb.cpu().numpy(), rb)
    # a rate chosen per frame through the facade equals the coder's call on the facade's mel
    mel = model.mel_spectrogram(x)
    c2, b2, _ = model.bvrnn.encode_vbr(mel, (17, 35, 64), tau, torch.zeros(1, 2, 1024, device=DEV))
    assert torch.equal(c2, codes) and torch.equal(b2, bits)


# ---------------------------------------------------------------------------------------------- 6: refusals from the library
def raw_call(model, B=2, T=4, ladder=(16, 32), short=0):
    eng = model.engine()
    lib = eng.lib
    H, Z = model.conf["h_dim"], model.conf["z_dim"]
    K = len(ladder)
    y, tau = torch.zeros(B, T, X, device=DEV), torch.zeros(B, T, device=DEV)
    codes, bits = torch.empty(B, T, Z, device=DEV), torch.empty(B, T, device=DEV)
    need = lib.bvc_vbr_workspace_bytes(eng.handle, B, T, min(max(K, 1), 8))
    assert need > lib.bvc_workspace_bytes(eng.handle, B, T) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lad = (ctypes.c_int32 * max(K, 1))(*ladder)
    with torch.cuda.device(DEV):
        rc = lib.bvc_bvrnn_encode_vbr(eng.handle, _abi.ptr(y), _abi.ptr(tau), lad, K, None, B, T, _abi.ptr(codes), _abi.ptr(bits), None, None,
                                      None, None, None, ctypes.c_void_p(ws.data_ptr()), need - short, eng.stream())
    torch.cuda.synchronize()
    return rc, lib.bvc_last_error().decode()


def test_library_refusals():
    var = model_of(128, "wide")
    assert raw_call(var)[0] == 0
    for ladder in ((32, 16), (16, 16), (-1, 16), (16, 65), (), tuple(range(9))):
        rc, msg = raw_call(var, ladder=ladder)
        assert rc == BVC_EINVAL and ("rung" in msg), (ladder, rc, msg)
    rc, msg = raw_call(var, short=1)
    assert rc == BVC_EINVAL and "workspace too small" in msg, (rc, msg)
    fix = model_of(128, "wide", var_bit=False)
    rc, msg = raw_call(fix)
    assert rc == BVC_EINVAL and "fixed-rate" in msg, (rc, msg)
    assert fix.engine().lib.bvc_vbr_workspace_bytes(fix.engine().handle, 2, 4, 9) == 0
