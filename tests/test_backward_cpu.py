"""The backward pass without a GPU: the weight-gradient entry point is declared in the header, bound in _abi.SIGNATURES, exported by
the built library at ABI 3, and refuses a bad shape or a missing or misaligned matrix on the host, before anything touches a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BVC_EINVAL = -1


def test_weight_grad_symbol_is_declared_bound_and_exported():
    from bvcodec import _abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvcodec.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+bvc_test_weight_grad\s*\(([^)]*)\)", hdr)
    assert m, "bvc_test_weight_grad is not declared in include/bvcodec.h"
    res, args = _abi.SIGNATURES["bvc_test_weight_grad"]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(","))
    lib = _abi.load()
    assert hasattr(lib, "bvc_test_weight_grad") and lib.bvc_abi_version() == 3


def test_weight_grad_refuses_on_the_host():
    from bvcodec import _abi
    lib = _abi.load()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    cut = (ctypes.c_int64 * 2)(-7, -7)
    for M, N, K in ((0, 64, 64), (-1, 64, 64), (4, 0, 64), (4, 64, 0), (4, 72, 64), (4, 64, 8), (4, 65, 64), (4, 64, 1000)):
        assert lib.bvc_test_weight_grad(p, p, M, N, K, p, cut, None) == BVC_EINVAL, (M, N, K)
        assert b"bvc_test_weight_grad" in lib.bvc_last_error() and b"multiples of 16" in lib.bvc_last_error()
    for dy, x, dw in ((None, p, p), (p, None, p), (p, p, None), (off, p, p), (p, off, p), (p, p, off)):
        assert lib.bvc_test_weight_grad(dy, x, 4, 64, 64, dw, cut, None) == BVC_EINVAL
        assert b"16-byte aligned" in lib.bvc_last_error()
    assert tuple(cut) == (-7, -7)                  # a refused call reports no cut


# ---------------------------------------------------------------------------------------------- the backward pass
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_oracle as bo  # noqa: E402
import bvrnn_draws as bd  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("bvc_bvrnn_backward", "bvc_bvrnn_backward_workspace_bytes", "bvc_bvrnn_backward_prepare", "bvc_bvrnn_grad_layout",
               "bvc_test_weight_grad")


def test_backward_symbols_are_declared_bound_and_exported():
    from bvcodec import _abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvcodec.h")).read(), flags=re.S)
    lib = _abi.load()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in include/bvcodec.h"
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(lib, name), name
    assert lib.bvc_abi_version() == 3
    assert lib.bvc_bvrnn_backward_workspace_bytes(None, 4, 10) == 0
    assert lib.bvc_bvrnn_backward(None, None, None, None, 1, 0, None, 2, 3, None, 1.0, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.bvc_bvrnn_backward_prepare(None, None) == -1


@pytest.mark.parametrize("h_dim,z_dim", ((64, 64), (1024, 64), (256, 32)))
def test_grad_layout_is_the_state_dict(h_dim, z_dim):
    from bvcodec import _abi, synth
    conf = bd.conf_of(h_dim, True, z_dim)
    sd = synth.bvrnn_state_dict(conf, 3)
    cfg = _abi.BvcConfig()
    cfg.num_mels, cfg.h_dim, cfg.z_dim = 80, h_dim, z_dim
    lib = _abi.load()
    n, total = ctypes.c_int32(0), ctypes.c_int64(0)
    assert lib.bvc_bvrnn_grad_layout(ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), ctypes.byref(total)) == 0 and n.value == 36
    names, offs, nums = (ctypes.c_char_p * 36)(), (ctypes.c_int64 * 36)(), (ctypes.c_int64 * 36)()
    assert lib.bvc_bvrnn_grad_layout(ctypes.byref(cfg), names, offs, nums, 35, None, None) == BVC_EINVAL
    assert lib.bvc_bvrnn_grad_layout(None, None, None, None, 0, None, None) == BVC_EINVAL
    assert lib.bvc_bvrnn_grad_layout(ctypes.byref(cfg), names, offs, nums, 36, None, None) == 0
    got = {names[i].decode(): int(nums[i]) for i in range(36)}
    assert got == {k: sd[k].numel() for k in bo.trainable(sd)}
    spans = sorted((int(offs[i]), int(nums[i])) for i in range(36))
    assert spans[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == total.value


def fixture_modes():
    for name, modes in (("h64_var", (0, 1)), ("h64_var_2", (2, 3)), ("h1024_var", (0, 2))):
        fx = np.load(os.path.join(GOLDEN, f"g13_bvrnn_backward_{name}.npz"))
        for mode in modes:
            k = f"m{mode}_"
            t = lambda n: torch.from_numpy(fx[k + n])
            greedy = bool(fx[k + "greedy"])
            yield name, mode, fx, dict(y=t("y"), bits=t("bits"), r=t("r"), noise=None if greedy else t("noise"), gdec=t("gdec"),
                                       gkld=float(fx[k + "gkld"]), p_use_gen=float(fx[k + "p_use_gen"]), greedy=greedy)


def test_oracle_gives_the_reference_gradients():
    """The oracle at float32 against the reference's own gradients (tests/golden/make_golden_backward.py), at the bar of the GPU tests:
    max|oracle32 - g64| <= 8 x max(max|reference - g64|, 2^-24 max|g64|).  Measured: identical bits.  The fixtures keep the margins."""
    from bvcodec import synth
    for name, mode, fx, c in fixture_modes():
        assert os.path.getsize(os.path.join(GOLDEN, f"g13_bvrnn_backward_{name}.npz")) <= 1 << 20
        h_dim = 64 if name.startswith("h64") else 1024
        sd = synth.bvrnn_state_dict(bd.conf_of(h_dim), int(fx["seed"]))
        args = (sd, c["y"], c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], c["gdec"], c["gkld"])
        g64, f64 = bo.grads(*args, torch.float64)
        g32, f32 = bo.grads(*args, torch.float32)
        rm, cm = bo.margins(f64, c["bits"], 64)
        assert rm >= bo.ROUND_MARGIN and cm >= bo.CLIP_MARGIN, (name, mode, rm, cm)
        assert torch.equal(f32["z"].double(), f64["z"])
        assert bool((c["bits"] == 0).any()) and bool((c["bits"] == 64).any())
        for k in g64:
            if f"m{mode}_g_{k}" in fx.files:
                pick, ref = (lambda t: t.reshape(1, -1)), torch.from_numpy(fx[f"m{mode}_g_{k}"])
            else:
                idx = torch.from_numpy(bo.entries(g64[k].numel()))
                pick, ref = (lambda t: t.reshape(-1)[idx].reshape(1, -1)), torch.from_numpy(fx[f"m{mode}_e_{k}"])
                assert abs(float(g32[k].double().norm()) - float(fx[f"m{mode}_n_{k}"])) <= 1e-6 * float(fx[f"m{mode}_n_{k}"])
            v = bd.compare(pick(g32[k]).double().numpy(), pick(g64[k]).numpy(), ref.double().reshape(1, -1).numpy(), f"{name} mode {mode} {k}")
            assert v.ok, v.message


def test_selected_cases_keep_the_margins():
    """The condition under which no GPU case is cut or skipped: in the float64 oracle every rounded argument of an active bit is at
    least 2e-5 from 0.5 and every e, 1 - e, prior, 1 - prior under the mask at least 1e-5 from the clip; the float32 oracle then
    rounds the same samples.  The list covers what it is written to cover."""
    from bvcodec import synth
    cases = bo.CASES
    assert len(set(cases)) == len(cases)
    for h in (64, 1024):
        assert {(B, T) for c in cases if c[0] == h for B, T in [c[3:5]]} >= {(B, T) for B in (1, 3, 17) for T in (1, 2, 7)}
        assert {c[5] for c in cases if c[0] == h} == {0, 1, 2, 3} and {c[2] for c in cases if c[0] == h} == {True, False}
        assert {c[1] for c in cases if c[0] == h} == {"default", "wide"} and {c[6] for c in cases if c[0] == h} == {"random", 0, 35, 64}
    assert {c[0] for c in cases} == {64, 256, 512, 1024}
    switched = 0
    for case in cases:
        sd = synth.bvrnn_state_dict(bd.conf_of(case[0], case[2]), 1234, gains=bd.GAINS[case[1]])
        s = bo.select(case, sd)
        assert s["margins"][0] >= bo.ROUND_MARGIN and s["margins"][1] >= bo.CLIP_MARGIN, (bo.case_id(case), s["margins"])
        use = (s["r"] < s["p_use_gen"])
        switched += int(bool(use.any()) and not bool(use.all()))
    assert switched >= 4                   # frames of one call conditioned on both chains


def test_oracle_gradients_are_the_central_differences():
    """grads of the float64 oracle against central differences of the loss, on seeded entries of every tensor at h_dim 64, with the
    straight-through sample written as the smooth function it is differentiated as (forward's ``ste``).  The same comparison on a
    perturbed copy of the gradients fails."""
    from bvcodec import synth
    case = (64, "default", True, 3, 5, 2, "random")
    sd = synth.bvrnn_state_dict(bd.conf_of(64), 1234)
    c = bo.select(case, sd)
    g64, f64 = c["g64"], c["f64"]
    ste = torch.round(f64["arg"]) - f64["prob"]
    p0 = {k: v.double().clone() for k, v in sd.items() if k != "log_sigma"}
    gdec = c["gdec"].double()

    def loss(p, y):
        with torch.no_grad():
            o = bo.forward(p, y, c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], ste=ste)
        return float((o["dec"] * gdec).sum() + o["kld"] * c["gkld"])

    rng = np.random.default_rng(4)
    eps, worst, worst_bad = 1e-6, 0.0, 0.0
    for k in list(g64):
        base = c["y"].double() if k == "y" else p0[k]
        for idx in rng.choice(base.numel(), 2, replace=False):
            vals = []
            for sgn in (1.0, -1.0):
                moved = base.clone()
                moved.view(-1)[idx] += sgn * eps
                vals.append(loss(p0, moved) if k == "y" else loss(dict(p0, **{k: moved}), c["y"].double()))
            fd = (vals[0] - vals[1]) / (2 * eps)
            g = float(g64[k].reshape(-1)[idx])
            scale = max(abs(g), float(g64[k].abs().max()) * 1e-3, 1e-9)
            worst = max(worst, abs(fd - g) / scale)
            worst_bad = max(worst_bad, abs(fd - 1.01 * g) / scale)
    assert worst < 1e-4, worst                  # O(eps^2) truncation + 1e-16 / eps rounding of a loss of order 100
    assert worst_bad > 1e-3, worst_bad          # one percent off is seen


def test_backward_argument_checks_come_before_the_library(tmp_path, conf_var):
    from bvcodec import BVRNNCodecModel, config, synth
    p1, p2 = synth.write_checkpoints(conf_var, str(tmp_path), seed=7)
    m = BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).bvrnn
    B, T = 2, 3
    y, bits, gd = torch.zeros(B, T, 80), torch.full((B, T), 35.0), torch.zeros(B, T, 80)
    ok = dict(r=torch.zeros(T), noise=torch.zeros(B, T, 64))
    for bad in (dict(grad_dec=torch.zeros(B, T, 79)), dict(grad_dec=torch.zeros(B, T)), dict(grad_dec=None), dict(grad_kld=torch.zeros(2)),
                dict(grad_kld=torch.zeros(1)), dict(grad_kld="1"), dict(grad_kld=None), dict(r=torch.zeros(T + 1)), dict(noise=torch.zeros(B, T, 63)),
                dict(noise=torch.zeros(T, B, 64)), dict(varBitrate=None), dict(varBitrate=torch.zeros(B, T + 1)), dict(y=torch.zeros(B, T, 81)),
                dict(y=torch.zeros(B, 80))):
        kw = dict(dict(y=y, varBitrate=bits, grad_dec=gd, grad_kld=1.0), **ok)
        kw.update(bad)
        with pytest.raises(ValueError, match="backward:"):
            m.backward(kw.pop("y"), 0.5, False, kw.pop("varBitrate"), kw.pop("grad_dec"), kw.pop("grad_kld"), **kw)
    with pytest.raises(ValueError, match="forward_train"):
        m.forward_train(y, 0.5, True, bits, {"mean_mel": torch.zeros(80)})
    layout, total = m.grad_layout()
    assert len(layout) == 36 and total == sum(n for _, _, n in layout) and {n for n, _, _ in layout} == set(m.grad_parameters())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.backward(y, 0.5, False, bits, gd, 1.0, **ok)
