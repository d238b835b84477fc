"""What test_gpu_coder_sizes.py relies on, shown without a GPU: at every (h_dim, z_dim, B, T) of the size table the float32 oracle's
own rounded outputs stay inside the caps of the tie rule against the float64 oracle (a condition of the comparison, not a
measurement: a case that breaks one gets a seed of its own in bvrnn_draws.SEEDS), the two config checks - config.check_supported and
the library's check_config - say the same of every size of the table and of a few that are refused, and the size rules the GPU tests
branch on (which entry point refuses which size) are the library's, read from its source."""
import ctypes
import os
import re

import pytest
import torch

import bvrnn_draws as bd
from bvcodec import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bernoulli-var-speech-codec_amd", "csrc")


@pytest.mark.parametrize("h_dim,z_dim,B,T", bd.SIZE_CASES)
@pytest.mark.parametrize("draw", bd.SIZE_DRAWS)
def test_float32_oracle_meets_the_tie_caps_at_every_size(draw, h_dim, z_dim, B, T):
    ref = bd.reference(draw, h_dim, B, T, z_dim)
    assert tuple(ref["codes"].shape) == (B, T, z_dim) and tuple(ref["o64"]["encode"]["all_h"].shape) == (B, T, h_dim)
    assert float(ref["bits"].max()) <= z_dim and tuple(ref["mask"].shape) == (B, T, z_dim)
    g = bd.regime(draw, h_dim, B, T, z_dim)
    print(f"REGIME draw={draw} h_dim={h_dim} z_dim={z_dim} B={B} T={T} seed={bd.seed_of(h_dim, draw, z_dim)} " + " ".join(f"{k}={v:.4g}" for k, v in g.items()))
    for name, cut in ref["cuts32"].items():
        print(cut)
        cut.check()


def test_the_size_table_covers_its_classes():
    sizes = [(h, z) for _, h, z, _ in bd.SIZE_CLASSES]
    assert len(set(sizes)) == len(sizes) == 14
    assert all(h % 16 == 0 and z % 16 == 0 for h, z in sizes)
    assert set(bd.PINNED_SIZES) <= set(sizes) and set(bd.WIRE_SIZES) <= set(sizes)
    for key in bd.SEEDS:
        assert key[:1] + key[2:] in {(h, z) for h, z in sizes} | {(256, 64)}, key
    # every branch of the size rules is taken by some row
    assert {bd.flow_supported(h, z) for h, z in sizes} == {True, False}
    assert {bd.forward_runs(h, z) for h, z in sizes} == {True, False} and {bd.conceal_runs(h, z) for h, z in sizes} == {True, False}
    assert {bd.forward_fallback_runs(h, z) for h, z in sizes if bd.forward_runs(h, z)} == {True, False}
    assert {h // 16 for h, z in sizes if h < 128} == {1, 3, 4, 7} and {z // 16 for h, z in sizes} == {1, 2, 3, 4, 6, 8, 9}


def test_the_size_rules_are_the_librarys():
    """flow_supported / forward_runs / conceal_runs restate conditions of the sources: the conditions and the messages are there."""
    rec = open(os.path.join(CSRC, "recurrence.hip")).read()
    flow = open(os.path.join(CSRC, "k_flow.hip")).read()
    model = open(os.path.join(CSRC, "model.hip")).read()
    assert f'if (Z > H) {{ set_error("{bd.FORWARD_REFUSAL}")' in rec
    assert f'if (!d_z && Z > X && 2 * Z > H) {{ set_error("{bd.FORWARD_NEEDS_Z}")' in rec
    assert f'if (m->cfg.z_dim > 3 * m->cfg.h_dim) {{ set_error("{bd.CONCEAL_REFUSAL}")' in rec
    assert "if (Z > 128 || X > 128) m->flow_perh = 0;" in model
    body = flow[flow.index("int flow_perh(int h_dim) {"):]
    body = body[:body.index("}\n") + 1]
    assert re.findall(r"h_dim == (\d+)\) return (\d+)", body) == [("128", "1"), ("256", "2"), ("512", "4"), ("1024", "8")]
    assert "if (h_dim < 128) return 1;" in body and body.rstrip().endswith("return 0;\n}".strip())


def library_verdict(h_dim, z_dim):
    """The C check_config through bvc_model_create with one dummy tensor: BVC_EINVAL (-1) with a message if the config is refused;
    anything else - no device (-5) here, a missing tensor (-4) on a machine with one - means the config passed."""
    from bvcodec import _abi
    import numpy as np
    lib = _abi.load()
    cfg = _abi.BvcConfig()
    cfg.num_mels, cfg.h_dim, cfg.z_dim, cfg.var_bit = 80, h_dim, z_dim, 1
    cfg.n_fft, cfg.hop, cfg.pad_left, cfg.sample_rate = 1024, 256, 256, 22050
    cfg.upsample_initial_channel, cfg.n_up, cfg.n_resk = 128, 4, 3
    for i, (u, k) in enumerate(((8, 16), (8, 16), (2, 4), (2, 4))):
        cfg.up_rates[i], cfg.up_kernels[i] = u, k
    t = (_abi.BvcTensor * 1)()
    dummy = np.zeros(4, dtype=np.float32)
    t[0].name, t[0].h_data, t[0].numel = b"mean_mel", dummy.ctypes.data, 4
    h = ctypes.c_void_p()
    rc = lib.bvc_model_create(ctypes.byref(cfg), t, 1, ctypes.byref(h))
    assert rc != 0 and not h.value
    return rc != -1, (lib.bvc_last_error() or b"").decode()


def host_verdict(h_dim, z_dim):
    conf = config.load_config(config.DEFAULT_CONFIG)
    conf["h_dim"], conf["z_dim"] = h_dim, z_dim
    try:
        config.check_supported(conf)
    except ValueError as e:
        return False, str(e)
    return True, ""


@pytest.mark.parametrize("h_dim,z_dim", [(h, z) for _, h, z, _ in bd.SIZE_CLASSES])
def test_both_config_checks_accept_every_size_of_the_table(h_dim, z_dim):
    assert host_verdict(h_dim, z_dim) == (True, "")
    ok, msg = library_verdict(h_dim, z_dim)
    assert ok, msg


@pytest.mark.parametrize("h_dim,z_dim", bd.REJECTED_SIZES)
def test_both_config_checks_refuse_the_same_sizes(h_dim, z_dim):
    ok, msg = host_verdict(h_dim, z_dim)
    assert not ok and "multiples of 16" in msg
    ok, msg = library_verdict(h_dim, z_dim)
    assert not ok and "multiples of 16" in msg
