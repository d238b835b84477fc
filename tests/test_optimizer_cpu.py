"""The optimiser without a GPU: the numpy oracle of the step (tests/optimizer_oracle.py) is torch.optim.AdamW with clip_grad_norm_; the
new entry points are declared in the header, bound in _abi.SIGNATURES and exported at ABI 3, and refuse null arguments on the host
before anything touches a device; the Python AdamW rejects bad hyperparameters and unknown names before it needs an engine; the
float64 training loop of the "it learns" case falls by the factor the GPU test is held to half of."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvrnn_draws as bd  # noqa: E402
import optimizer_oracle as oo  # noqa: E402

BVC_EINVAL = -1
NEW_SYMBOLS = ("bvc_bvrnn_params_get", "bvc_bvrnn_params_set", "bvc_optimizer_create", "bvc_optimizer_destroy", "bvc_optimizer_step",
               "bvc_optimizer_state_get", "bvc_optimizer_state_set", "bvc_test_folded_hop")


def small_params(seed=0):
    rng = np.random.default_rng(seed)
    return {"a.weight": torch.from_numpy(rng.standard_normal((16, 32))), "a.bias": torch.from_numpy(rng.standard_normal(16)),
            "b.weight": torch.from_numpy(0.01 * rng.standard_normal((48, 16)))}


@pytest.mark.parametrize("weight_decay", (0.0, 0.1))
@pytest.mark.parametrize("max_grad_norm", (0.0, 1.0))
def test_oracle_is_torch_adamw_with_clip_grad_norm(weight_decay, max_grad_norm):
    """Five steps at float64 against torch.optim.AdamW (+ clip_grad_norm_) on CPU float64 tensors, to 1e-12 relative: parameters, both
    moments and the returned norm.  Gradients of mixed scales, one tensor's all zero at one step."""
    params = small_params()
    rng = np.random.default_rng(1)
    seq = []
    for s in range(5):
        g = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)) * 10.0 ** rng.uniform(-3, 1, tuple(v.shape))) for k, v in params.items()}
        if s == 2:
            g["a.bias"] = torch.zeros_like(g["a.bias"])
        seq.append(g)
    hyper = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    o = oo.AdamWOracle(params, np.float64)
    norms = [o.step(g, **hyper) for g in seq]
    p, m, v, tnorms = oo.torch_adamw(params, seq, **hyper)
    assert np.allclose(norms, tnorms, rtol=1e-12, atol=0)
    assert max_grad_norm == 0 or max(norms) > 10 * max_grad_norm          # the clip is active
    for got, want in ((o.p, p), (o.m, m), (o.v, v)):
        for k in params:
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    moved = max(np.abs(o.p[k] - params[k].numpy()).max() for k in params)
    assert moved > 0.1                                                    # the updates are a visible share of the weights


def test_float32_oracle_follows_the_float64_one():
    params = {k: v.float() for k, v in small_params().items()}
    g = oo.synthetic_grads({k: tuple(v.shape) for k, v in params.items()}, 3)
    o64, o32 = oo.AdamWOracle(params, np.float64), oo.AdamWOracle(params, np.float32)
    for _ in range(3):
        n64, n32 = o64.step(g, 0.05, weight_decay=0.1, max_grad_norm=1.0), o32.step(g, 0.05, weight_decay=0.1, max_grad_norm=1.0)
        assert n64 == n32                                # the norm is a float64 sum of the float32 gradients in both
    for k in params:
        assert o32.p[k].dtype == np.float32 and np.abs(o32.p[k] - o64.p[k]).max() <= 1e-5 * max(1.0, np.abs(o64.p[k]).max())


def test_synthetic_gradients_have_the_edge_cases():
    conf = bd.conf_of(64)
    from bvcodec import synth
    sd = synth.bvrnn_state_dict(conf, 1234)
    shapes = {k: tuple(v.shape) for k, v in sd.items() if k not in ("mean_mel", "std_mel", "log_sigma")}
    g = oo.synthetic_grads(shapes, 5)
    assert set(g) == set(shapes) and len(g) == 36
    assert not bool(g[oo.ZERO_TENSOR].any()) and int((g[oo.ONE_ELEMENT_TENSOR] != 0).sum()) == 1
    mags = torch.cat([v.abs().reshape(-1) for v in g.values()])
    nz = mags[mags > 0]
    assert float(nz.min()) >= 0.99e-12 and float(nz.max()) > 10.0 and float(nz.median()) < 1e-1


def test_optimizer_symbols_are_declared_bound_and_exported():
    from bvcodec import _abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bvcodec.h")).read(), flags=re.S)
    lib = _abi.load()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in include/bvcodec.h"
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(lib, name), name
    assert lib.bvc_abi_version() == 3
    assert ctypes.sizeof(_abi.BvcAdamWConfig) == 48 and re.search(r"double\s+lr,\s*beta1,\s*beta2,\s*eps,\s*weight_decay,\s*max_grad_norm;", hdr)


def test_null_arguments_are_refused_on_the_host():
    from bvcodec import _abi
    lib = _abi.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    cfg = _abi.BvcAdamWConfig(1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
    out = ctypes.c_void_p(1)
    step = ctypes.c_int64(0)
    assert lib.bvc_bvrnn_params_get(None, p, None) == BVC_EINVAL and b"null model" in lib.bvc_last_error()
    assert lib.bvc_bvrnn_params_set(None, p, None) == BVC_EINVAL and b"null model" in lib.bvc_last_error()
    assert lib.bvc_optimizer_create(None, ctypes.byref(out)) == BVC_EINVAL and out.value is None
    assert lib.bvc_optimizer_create(None, None) == BVC_EINVAL
    assert lib.bvc_optimizer_step(None, ctypes.byref(cfg), p, None, None) == BVC_EINVAL and b"null optimizer" in lib.bvc_last_error()
    assert lib.bvc_optimizer_state_get(None, ctypes.byref(step), p, p, None) == BVC_EINVAL
    assert lib.bvc_optimizer_state_set(None, ctypes.byref(step), p, p, None) == BVC_EINVAL
    assert lib.bvc_test_folded_hop(None, p, p, None) == BVC_EINVAL
    lib.bvc_optimizer_destroy(None)


@pytest.fixture(scope="module")
def bvrnn(tmp_path_factory):
    from bvcodec import BVRNNCodecModel, config, synth
    conf = config.load_config(config.DEFAULT_CONFIG)
    p1, p2 = synth.write_checkpoints(conf, str(tmp_path_factory.mktemp("opt")), seed=7)
    return BVRNNCodecModel(config.DEFAULT_CONFIG, p1, p2).bvrnn


@pytest.mark.parametrize("bad", (dict(lr=-1e-3), dict(lr=float("nan")), dict(lr="1e-3"), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                                 dict(betas=(0.9,)), dict(betas=0.9), dict(eps=0.0), dict(eps=-1e-8), dict(weight_decay=-0.1),
                                 dict(max_grad_norm=-1.0), dict(lr=True)))
def test_python_adamw_rejects_bad_hyperparameters(bvrnn, bad):
    with pytest.raises(ValueError, match="AdamW: invalid"):
        bvrnn.optimizer(**bad)
    opt = bvrnn.optimizer()
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay, opt.max_grad_norm) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.0)
    for k, v in bad.items():
        setattr(opt, k, v)
    with pytest.raises(ValueError, match="AdamW: invalid"):            # the attributes are read at every step
        opt.step({})


def test_python_adamw_rejects_unknown_names_and_shapes(bvrnn):
    opt = bvrnn.optimizer()
    good = bvrnn.grad_parameters()
    with pytest.raises(ValueError, match="no trainable tensors"):
        opt.step({"mean_mel": torch.zeros(80)})
    with pytest.raises(ValueError, match="no trainable tensors"):
        opt.step({"enc.0.weight": good["enc.0.weight"]}, params={"bogus": torch.zeros(1)})
    with pytest.raises(ValueError, match="'enc.0.bias' must be a tensor"):
        opt.step({"enc.0.bias": torch.zeros(3)})
    with pytest.raises(ValueError, match="flat tensor"):
        opt.step(torch.zeros(7))
    with pytest.raises(ValueError, match="flat tensor"):
        opt.step(None)
    with pytest.raises(ValueError, match="no trainable tensors"):
        bvrnn.load_parameters({"std_mel": torch.ones(80)})
    with pytest.raises(ValueError, match="'phi_x.0.weight' must be a tensor"):
        bvrnn.load_parameters({"phi_x.0.weight": torch.zeros(80, 1024)})
    with pytest.raises(ValueError, match="load_state_dict"):
        opt.load_state_dict({"step": 1})
    with pytest.raises(ValueError, match="step must be"):
        opt.load_state_dict({"step": -1, "state": {}})
    with pytest.raises(ValueError, match="is missing"):
        opt.load_state_dict({"step": 1, "state": {"enc.0.bias": {"exp_avg": torch.zeros(1024)}}})
    with pytest.raises(ValueError, match="flat=True"):
        bvrnn.backward(torch.zeros(2, 3, 80), 0.5, True, torch.full((2, 3), 35.0), torch.zeros(2, 3, 80), 1.0, grad_input=True, flat=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step(good)


def test_float64_loop_learns():
    """The "it learns" case at float64 (tests/backward_oracle.py + the oracle step): the loss falls by at least LEARN_FALL in 30
    steps.  The GPU test (tests/test_gpu_optimizer.py) asserts sqrt(LEARN_FALL) of the library's loop."""
    curve = oo.learn_curve_oracle()
    print("float64 curve:", " ".join(f"{v:.4g}" for v in curve))
    assert len(curve) == oo.LEARN_STEPS + 1 and all(np.isfinite(curve))
    assert curve[0] / curve[-1] >= oo.LEARN_FALL, (curve[0], curve[-1])
    assert curve[0] / min(curve) < 2 * oo.LEARN_FALL          # the threshold sits below what was seen, not far below
