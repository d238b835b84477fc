"""The weight-gradient kernel of the backward pass alone (csrc/k_backward.hip), through bvc_test_weight_grad: dW = dY^T X against the
float64 product at the project's bar (vocoder_layers.compare: max|hip - g64| <= 8 x max(e32, 2^-24 max|g64|), e32 the error of torch's
own float32 product on the CPU), at the row counts where the cut into chunks and 128-row blocks has an edge - one row, fewer rows
than an MFMA step, one staging trip and one row more, no full block, several blocks with a short last one, several chunks - and at
the weight shapes of the coder: a single output tile, 80 columns or 80 rows (a tile cut at 16 of its 64), the GRU's 3H x H.  Every
output is written and nothing behind it; two calls give the same bits; a wrong chunk seam or lane map shows orders of magnitude above
the bar where all of dY but one row, or but one column, is zero.  Measured ratios: profiles/backward_parity.md.  Needs the MI355X:
run with ``-m gpu``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bvrnn_draws as bd
from gpu_common import DEV

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 16, 17, 100, 1000, 11129)
SHAPES = ((64, 64), (1024, 80), (80, 1024), (64, 1024), (1024, 2048), (3072, 1024))        # (N, K) of dW
CANARY_ROWS, CANARY = 16, 777.0
LEDGER = bd.Ledger("weight gradient")
from backward_oracle import BLOCK, want_cut  # noqa: E402  (weight_grad_cut restated, shared with the CPU tests of the case tables)


@pytest.fixture(scope="module")
def lib():
    from bvcodec import _abi
    return _abi.load()


def weight_grad(lib, dy, x, M, N, K):
    """One call on device operands -> (dW on the device, (chunks, rows per chunk)); all of dW written, nothing behind it."""
    from bvcodec import _abi
    buf = torch.full((N + CANARY_ROWS, K), float("nan"), device=DEV)
    buf[N:] = CANARY
    cut = (ctypes.c_int64 * 2)()
    _abi.check(lib.bvc_test_weight_grad(_abi.ptr(dy), _abi.ptr(x), M, N, K, _abi.ptr(buf), cut, _abi.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    out = buf[:N]
    assert bool(torch.isfinite(out).all()), f"{int((~torch.isfinite(out)).sum())} elements not written (or not finite)"
    assert bool((buf[N:] == CANARY).all()), "rows behind the output were written"
    return out, (int(cut[0]), int(cut[1]))


@functools.lru_cache(maxsize=2)
def draw(M, N, K):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    return torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)


def check(lib, dy, x, what):
    M, N = dy.shape
    K = x.shape[1]
    ref64 = dy.double().t() @ x.double()
    ref32 = dy.t() @ x
    dyd, xd = dy.to(DEV), x.to(DEV)
    got, cut = weight_grad(lib, dyd, xd, M, N, K)
    assert cut == want_cut(M, N, K), (cut, want_cut(M, N, K))
    again, _ = weight_grad(lib, dyd, xd, M, N, K)
    assert torch.equal(got, again), f"{what}: two calls differ in {int((got != again).sum())} elements"
    v = bd.compare(got.cpu().numpy(), ref64.numpy(), ref32.numpy(), what)
    print(f"RATIO {what} chunks={cut[0]} rows={cut[1]} ratio={v.ratio:.3f} e_hip={v.e_hip:.3e} e32={v.e32:.3e}", flush=True)
    LEDGER.add(f"N={N} K={K}", v)
    assert v.ok, v.message


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", ROWS)
def test_weight_grad_against_float64(lib, M, N, K):
    dy, x = draw(M, N, K)
    check(lib, dy, x, f"dW M={M} N={N} K={K}")


@pytest.mark.parametrize("N,K", ((64, 64), (1024, 80), (80, 1024)))
def test_weight_grad_one_row_and_one_column(lib, N, K):
    """M = 1000, four chunks of 256 rows: all of dY zero but row 777 (in the last chunk), then all but column N - 3.
    Every output is then one product, or one column's sum: rows taken twice, skipped or given to another lane are far above the bar."""
    M = 1000
    dy, x = draw(M, N, K)
    one_row = torch.zeros_like(dy)
    one_row[777] = dy[777]
    check(lib, one_row, x, f"dW one row M={M} N={N} K={K}")
    one_col = torch.zeros_like(dy)
    one_col[:, N - 3] = dy[:, N - 3]
    check(lib, one_col, x, f"dW one column M={M} N={N} K={K}")


def test_weight_grad_zero_gives_zero(lib):
    dy, x = draw(1000, 64, 1024)
    got, _ = weight_grad(lib, torch.zeros_like(dy).to(DEV), x.to(DEV), 1000, 64, 1024)
    assert not bool(got.any())


def test_cases_cover_both_paths_and_ledger():
    """The row counts reach the single-chunk path (written in place) and the chunked one (partial sums, ordered reduction), a chunk
    of one block and of several, and a last block that is short.  Prints the PARITY lines (profiles/backward_parity.md)."""
    cuts = {(M, N, K): want_cut(M, N, K) for M in ROWS for N, K in SHAPES}
    assert any(c[0] == 1 and M > BLOCK for (M, _, _), c in cuts.items()) and any(c[0] > 8 for c in cuts.values())
    assert any(c[1] == BLOCK for c in cuts.values()) and any(c[1] > BLOCK for c in cuts.values())
    assert all((c[0] - 1) * c[1] < M <= c[0] * c[1] for (M, _, _), c in cuts.items())
    LEDGER.close()


# ================================================================================================ the backward pass
# bvc_bvrnn_backward (model.bvrnn.backward) against tests/backward_oracle.py at float64.  The bar, per gradient tensor:
# max|hip - g64| <= 8 x max(e32, 2^-24 max|g64|), e32 = max|oracle32 - g64| of that case and tensor with the samples held equal
# (a fixture case: the reference's own float32 gradients in oracle32's place).  Every case first asserts that the HIP z equals the
# oracle's exactly; the cases are selected (backward_oracle.select, asserted on the CPU in test_backward_cpu.py) so that it must.
import os  # noqa: E402
import tempfile  # noqa: E402

import backward_oracle as bo  # noqa: E402
from gpu_common import make_model  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BWD_LEDGERS = {d: bd.Ledger(f"backward {d}") for d in ("default", "wide", "fixture")}


def family(name):
    return name.split(".")[0] + (" bias" if "bias" in name else "")


def model_of(h_dim, draw="default", var_bit=True):
    model, _, sd, _ = make_model(var_bit=var_bit, h_dim=h_dim, gains=bd.GAINS[draw])
    return model, sd


def hip_backward(model, c, gdec=None, gkld=None, grad_input=True):
    dev = lambda t: None if t is None else t.to(DEV)
    out = model.bvrnn.backward(dev(c["y"]), c["p_use_gen"], c["greedy"], dev(c["bits"]), dev(c["gdec"] if gdec is None else gdec),
                               c["gkld"] if gkld is None else gkld, r=c["r"], noise=c["noise"], grad_input=grad_input, return_forward=True)
    torch.cuda.synchronize()
    return out


def hold(got, g64, g32, what, ledger, names=None):
    """Every tensor of ``names`` (default: all of g64) to the bar; all failures of the case are reported.  ledger: a key of BWD_LEDGERS,
    or a Ledger."""
    ledger = BWD_LEDGERS[ledger] if isinstance(ledger, str) else ledger
    bad = []
    for k in (g64 if names is None else names):
        v = bd.compare(got[k].detach().cpu().double().reshape(1, -1).numpy(), g64[k].reshape(1, -1).numpy(), g32[k].double().reshape(1, -1).numpy(),
                       f"{what} {k}")
        ledger.add(family(k), v)
        if not v.ok:
            bad.append(v.message)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", bo.CASES, ids=bo.case_id)
def test_backward_against_float64_oracle(case):
    h_dim, draw, var_bit = case[:3]
    model, sd = model_of(h_dim, draw, var_bit)
    c = bo.select(case, sd)
    got, fwd = hip_backward(model, c)
    assert torch.equal(fwd["z"].cpu().double(), c["f64"]["z"]), "the samples differ from the oracle's"
    g32, _ = bo.grads(sd, c["y"], c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], c["gdec"], c["gkld"], torch.float32,
                      z=c["f64"]["z"], var_bit=var_bit)
    assert set(got) == set(c["g64"]) and all(got[k].shape == c["g64"][k].shape for k in got)
    hold(got, c["g64"], g32, bo.case_id(case), draw)


def fixture_case(fx, mode):
    k = f"m{mode}_"
    t = lambda n: torch.from_numpy(fx[k + n])
    greedy = bool(fx[k + "greedy"])
    return dict(y=t("y"), bits=t("bits"), r=t("r"), noise=None if greedy else t("noise"), gdec=t("gdec"), gkld=float(fx[k + "gkld"]),
                p_use_gen=float(fx[k + "p_use_gen"]), greedy=greedy)


@pytest.mark.parametrize("name,modes", (("h64_var", (0, 1)), ("h64_var_2", (2, 3)), ("h1024_var", (0, 2))))
def test_backward_against_reference_fixtures(name, modes):
    """The reference's own BVRNN under autograd (tests/golden/make_golden_backward.py).  h_dim 64: every gradient in full.  h_dim 1024:
    the biases and the input gradient in full, the stored 4096 entries of every weight matrix, and its Frobenius norm:
    | ||hip|| - ||ref|| | <= ||hip - ref||_F <= sqrt(numel) max|hip - ref| <= sqrt(numel) (bar + e32), bar and e32 of the stored entries."""
    fx = np.load(os.path.join(GOLDEN, f"g13_bvrnn_backward_{name}.npz"))
    h_dim = 64 if name.startswith("h64") else 1024
    model, sd = model_of(h_dim)
    for mode in modes:
        c = fixture_case(fx, mode)
        g64, f64 = bo.grads(sd, c["y"], c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], c["gdec"], c["gkld"], torch.float64)
        got, fwd = hip_backward(model, c)
        assert torch.equal(fwd["z"].cpu().double(), f64["z"]), "the samples differ from the oracle's"
        full = [k for k in g64 if f"m{mode}_g_{k}" in fx.files]
        hold(got, g64, {k: torch.from_numpy(fx[f"m{mode}_g_{k}"]) for k in full}, f"{name} mode {mode}", "fixture", full)
        assert h_dim == 1024 or len(full) == len(g64)
        for k in (k for k in g64 if k not in full):
            idx = torch.from_numpy(bo.entries(g64[k].numel()))
            pick = lambda t: t.detach().cpu().reshape(-1)[idx]
            stored = torch.from_numpy(fx[f"m{mode}_e_{k}"])
            v = bd.compare(pick(got[k]).double().reshape(1, -1).numpy(), pick(g64[k]).reshape(1, -1).numpy(), stored.double().reshape(1, -1).numpy(),
                           f"{name} mode {mode} {k} entries")
            BWD_LEDGERS["fixture"].add(family(k), v)
            assert v.ok, v.message
            norm = float(got[k].detach().cpu().double().norm())
            room = np.sqrt(g64[k].numel()) * (v.bar + v.e32)
            assert abs(norm - float(fx[f"m{mode}_n_{k}"])) <= room, (k, norm, float(fx[f"m{mode}_n_{k}"]), room)


@pytest.mark.parametrize("case", ((64, "default", True, 3, 7, 2, "random"), (1024, "default", True, 17, 2, 1, "random"),
                                  (1024, "default", False, 3, 7, 3, "random")), ids=bo.case_id)
def test_backward_runs_the_forward_of_bvc_bvrnn_forward(case):
    """The forward outputs of the backward call are bvc_bvrnn_forward's bits on the same inputs (T on both sides of the all-frame
    MLPs' threshold of 4 frames)."""
    model, sd = model_of(*case[:3])
    c = bo.draw_inputs(case, 11)
    _, fwd = hip_backward(model, c)
    dec, kld, ex = model.bvrnn.forward(c["y"].to(DEV), c["p_use_gen"], c["greedy"], c["bits"].to(DEV), r=c["r"], noise=c["noise"], return_all=True)
    assert torch.equal(fwd["dec"], dec) and torch.equal(fwd["kld"], kld)
    for k in ("z", "prob", "prior", "kld_frames"):
        assert torch.equal(fwd[k], ex[k]), k


def test_backward_is_linear_and_deterministic():
    case = (1024, "default", True, 3, 7, 2, "random")
    model, sd = model_of(*case[:3])
    c = bo.select(case, sd)
    got, _ = hip_backward(model, c)
    a, _ = hip_backward(model, c, gkld=0.0)
    b, _ = hip_backward(model, c, gdec=torch.zeros_like(c["gdec"]))
    g32, _ = bo.grads(sd, c["y"], c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], c["gdec"], c["gkld"], torch.float32, z=c["f64"]["z"])
    hold({k: a[k].double() + b[k].double() for k in got}, c["g64"], g32, "sum of the two halves", "default")
    zero, _ = hip_backward(model, c, gdec=torch.zeros_like(c["gdec"]), gkld=0.0)
    assert all(not bool(v.any()) for v in zero.values()), [k for k, v in zero.items() if bool(v.any())]
    again, _ = hip_backward(model, c)
    assert all(torch.equal(got[k], again[k]) for k in got), "two calls differ"
    s2 = torch.cuda.Stream(DEV)
    s2.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s2):
        other, _ = hip_backward(model, c)                       # its own workspace: the engine keeps one per stream
    torch.cuda.current_stream(DEV).wait_stream(s2)
    assert all(torch.equal(got[k], other[k]) for k in got), "a call on a second stream differs"


@pytest.mark.parametrize("y_grad", (False, True))
def test_autograd_bridge(y_grad):
    """forward_train under an L1 reconstruction loss + 0.1 kld written in torch: .grad is backward(...)'s output fed with that loss's
    own gradients, bit for bit; y.grad is there exactly when asked for."""
    case = (64, "default", True, 3, 7, 2, "random")
    model, sd = model_of(*case[:3])
    c = bo.draw_inputs(case, 21)
    target = c["y"] + 0.3 * c["gdec"]
    loss_of = lambda dec, kld: (dec - target.to(dec.device)).abs().mean() + 0.1 * kld
    params = {k: v.requires_grad_(True) for k, v in model.bvrnn.grad_parameters().items()}
    assert set(params) == set(bo.trainable(sd)) - {"log_sigma"} and all(torch.equal(params[k].detach(), sd[k]) for k in params)
    y = c["y"].clone().requires_grad_(y_grad)
    dec, kld = model.bvrnn.forward_train(y, c["p_use_gen"], c["greedy"], c["bits"], params, r=c["r"], noise=c["noise"])
    loss_of(dec, kld).backward()
    assert (y.grad is not None) == y_grad
    d = dec.detach().clone().requires_grad_(True)
    k = kld.detach().clone().requires_grad_(True)
    loss_of(d, k).backward()
    want = model.bvrnn.backward(c["y"], c["p_use_gen"], c["greedy"], c["bits"], d.grad, float(k.grad), r=c["r"], noise=c["noise"], grad_input=y_grad)
    for name, p in params.items():
        assert p.grad is not None and torch.equal(p.grad, want[name]), name
    if y_grad:
        assert torch.equal(y.grad, want["y"])


def test_backward_refusals_leave_the_model_usable():
    from bvcodec import BVRNNCodecModel, _abi, config, synth
    conf = config.load_config(config.DEFAULT_CONFIG)
    d = tempfile.mkdtemp(prefix="bvc_test_noprior_")
    p1, p2 = synth.write_checkpoints(conf, d, seed=99)
    bare = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).to(DEV)
    for k in [k for k in bare._tensors if k.startswith("prior.")]:
        del bare._tensors[k]
    B, T = 3, 5
    y, bits = bd.inputs(B, T)
    y, bits = y.to(DEV), bits.to(DEV)
    gdec = torch.ones(B, T, 80, device=DEV)
    h0 = torch.zeros(1, B, 1024, device=DEV)
    layout_total = sum(int(np.prod(t.shape)) for k, t in bare._tensors.items() if k.split(".")[0] in ("phi_x", "phi_z", "enc", "dec", "rnn"))
    before = bare.bvrnn.encode(y, bits, h0)[0].clone()
    eng = bare.bvrnn.engine(y)
    flat = torch.empty(layout_total + 4 * 1024 * 1024, device=DEV)
    use = torch.zeros(T, dtype=torch.uint8)
    ws = torch.empty(int(eng.lib.bvc_bvrnn_backward_workspace_bytes(eng.handle, B, T)), dtype=torch.uint8, device=DEV)
    call = lambda e, uh, uh2, nbytes: e.lib.bvc_bvrnn_backward(e.handle, _abi.ptr(y), _abi.ptr(bits), _abi.ptr(use, torch.uint8), uh, uh2, None, B, T,
                                                             _abi.ptr(gdec), 1.0, _abi.ptr(flat), None, None, None, None, None, None,
                                                             _abi.ptr(ws, torch.uint8), nbytes, e.stream())
    assert call(eng, 1, 0, ws.numel()) == -4 and b"without the prior" in eng.lib.bvc_last_error()                # BVC_EMISSING
    assert torch.equal(bare.bvrnn.encode(y, bits, h0)[0], before)
    model, _ = model_of(1024)
    eng = model.bvrnn.engine(y)
    before = model.bvrnn.encode(y, bits, h0)[0].clone()
    need = int(eng.lib.bvc_bvrnn_backward_workspace_bytes(eng.handle, B, T))
    assert need > int(eng.lib.bvc_workspace_bytes(eng.handle, B, T))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert call(eng, 1, 0, need - 256) == -2 and b"workspace too small" in eng.lib.bvc_last_error()               # BVC_ENOMEM
    assert call(eng, 1, 0, int(eng.lib.bvc_workspace_bytes(eng.handle, B, T))) == -2
    assert call(eng, 0, 0, need) == -1 and b"at least one state must be updated" in eng.lib.bvc_last_error()
    assert call(eng, 0, 1, need) == -1 and b"never updated" in eng.lib.bvc_last_error()
    assert torch.equal(model.bvrnn.encode(y, bits, h0)[0], before)
    assert call(eng, 1, 0, need) == 0
    torch.cuda.synchronize()
    model.check_status()


def test_backward_parity_ledger():
    """Prints the PARITY lines of the backward comparisons (profiles/backward_parity.md)."""
    for led in BWD_LEDGERS.values():
        led.close()
