"""What test_gpu_bvrnn_draws.py relies on, shown on the CPU with the float64 oracle alone: gains=None leaves every checkpoint tensor
as it was, the three draws reach the regimes they are named for, the float32 oracle itself meets the tie caps at every shape and
seed the GPU tests use, and the closed forms of the pinned checkpoints are what the oracle computes from those checkpoints."""
import numpy as np
import pytest
import torch

import bvrnn_draws as bd
from bvcodec import synth
from oracle import bvrnn as obv


def test_gains_none_is_the_draw_as_it_was():
    for h_dim, var_bit, seed, mel_stats in ((1024, True, 1234, None), (64, True, 7, None), (128, False, 99, (-8.0, 0.05, 0.3))):
        conf = bd.conf_of(h_dim, var_bit)
        a = synth.bvrnn_state_dict(conf, seed, mel_stats)
        b = synth.bvrnn_state_dict(conf, seed, mel_stats, gains=None)
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k
    # (the stream of draws itself is pinned by the golden fixtures, which are decoded with these tensors)
    conf = bd.conf_of(64)
    a, w = synth.bvrnn_state_dict(conf, 1234), synth.bvrnn_state_dict(conf, 1234, gains=bd.GAINS["wide"])
    gh, go, gg = (np.float32(g) for g in bd.GAINS["wide"])
    for k in a:
        want = a[k] * gg if k.startswith("rnn.") else a[k] * (go if k.startswith(("enc.4.", "prior.4.")) else gh) if k.endswith((".weight", ".bias")) else a[k]
        assert torch.equal(w[k], want), k
    assert torch.equal(w["mean_mel"], a["mean_mel"]) and torch.equal(w["std_mel"], a["std_mel"]) and torch.equal(w["log_sigma"], a["log_sigma"])


@pytest.mark.parametrize("h_dim", bd.RANGE_HDIMS)
@pytest.mark.parametrize("draw", bd.DRAWS)
def test_draws_reach_their_regimes(draw, h_dim):
    B, T = (5, 48) if h_dim < 1024 else (20, 48)
    g = bd.regime(draw, h_dim, B, T)
    print(f"REGIME draw={draw} h_dim={h_dim} seed={bd.seed_of(h_dim, draw)} " + " ".join(f"{k}={v:.4g}" for k, v in g.items()))
    if draw == "default":
        assert g["max_logit"] < 0.5                     # what every other BVRNN test of the suite covers
    if draw == "wide":
        assert g["max_logit"] > 5 and g["max_h"] > 0.99
    if draw == "saturated":
        assert g["clamp_share"] >= 0.5 and g["exact01"] >= 0.01


@pytest.mark.parametrize("h_dim,B,T", bd.SHAPES)
@pytest.mark.parametrize("draw", bd.DRAWS)
def test_float32_oracle_meets_the_tie_caps(draw, h_dim, B, T):
    """The reference alone: the float32 oracle's rounded outputs equal the float64 oracle's outside the tie rule, within the caps."""
    ref = bd.reference(draw, h_dim, B, T)
    for name, cut in ref["cuts32"].items():
        print(cut)
        cut.check()


def test_reference_through_the_sized_signature_is_the_reference_as_it_was():
    """reference(..., z_dim=64) is the four-argument reference, and that one is what the harness computed before it took a z_dim:
    the shipped config's sizes, checkpoint seed 1234, inputs from generator 5 with bit counts in 0..64."""
    from bvcodec import config
    draw, h_dim, B, T = "default", 1024, 20, 48
    new = bd.reference(draw, h_dim, B, T, z_dim=64)
    assert new is bd.reference(draw, h_dim, B, T)
    conf = config.load_config(config.DEFAULT_CONFIG)
    assert conf["z_dim"] == 64 == bd.Z and bd.seed_of(h_dim, draw) == 1234 == bd.seed_of(h_dim, draw, 64)
    conf["h_dim"] = h_dim
    sd = synth.bvrnn_state_dict(conf, 1234, gains=None)
    rng = np.random.default_rng(5)
    y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32))
    bits = torch.from_numpy(rng.integers(0, 65, size=(B, T)).astype(np.float32))
    assert torch.equal(new["y"], y) and torch.equal(new["bits"], bits)
    for k in sd:
        assert torch.equal(new["sd"][k], sd[k]), k
    old = obv.encode(sd, y, bits, torch.zeros(B, h_dim), dtype=torch.float64)
    assert torch.equal(new["o64"]["encode"]["codes"], old["codes"]) and torch.equal(new["o64"]["encode"]["prob"], old["prob"])
    assert torch.equal(new["mask"], bits[:, :, None] > torch.arange(64, dtype=torch.float32)[None, None, :])


def test_logit_tables_keep_their_64_leading_values():
    t = np.array([s * v for v in bd.LOGIT_TABLE for s in (1.0, -1.0)], dtype=np.float32)
    rng = np.random.default_rng(11)
    be, bq = torch.from_numpy(t[rng.permutation(64)]), torch.from_numpy(t[rng.permutation(64)])
    a, b = bd.logit_tables()
    assert torch.equal(a, be) and torch.equal(b, bq)                # the 64-wide tables as they were
    for z in (16, 48, 64, 96, 128, 144):
        e, q = bd.logit_tables(z)
        n = min(z, 64)
        assert e.shape == q.shape == (z,) and torch.equal(e[:n], be[:n]) and torch.equal(q[:n], bq[:n])
        for i in range(64, z, 64):                                  # beyond 64: permutations of the 64-entry tables
            m = min(64, z - i)
            assert set(e[i:i + m].tolist()) <= set(be.tolist()) and set(q[i:i + m].tolist()) <= set(bq.tolist())
            if m == 64:
                assert sorted(e[i:i + 64].tolist()) == sorted(be.tolist()) and not torch.equal(e[i:i + 64], be)
        assert bd.pinned_bit_values(z)[3:5] == (z - 1.0, float(z)) and bd.pinned_bit_values(z)[:2] == (0.0, 1.0)
        assert z / 2 < bd.pinned_bit_values(z)[2] < z - 1 and bd.pinned_bit_values(z)[2] % 1 == 0.5
    assert bd.pinned_bit_values(64) == bd.PINNED_BITS == (0.0, 1.0, 34.5, 63.0, 64.0, 1000.0)
    assert bd.pinned_bit_values(48)[2] == 24.5


def test_teacher_forced_float32_oracle_meets_the_tie_caps():
    h_dim, B, T = bd.SHAPES[0]
    for draw in bd.DRAWS:
        ref = bd.reference(draw, h_dim, B, T)
        o = ref["o64"]["encode"]
        tf = obv.encode(ref["sd"], ref["y"], ref["bits"], torch.zeros(B, h_dim), forced_h=o["all_h"].float())
        fr = list(bd.TEACHER_FRAMES)
        cut = bd.Cut(f"{draw} teacher-forced float32 oracle", tf["codes"][:, fr], o["codes"][:, fr], o["prob"][:, fr], ref["mask"][:, fr].numpy())
        print(cut)
        cut.check()
        assert cut.rows_cut == 0 or cut.excluded <= 1


def test_pinned_logits_closed_form_is_what_the_oracle_computes():
    h_dim, B, T = 64, 5, 3
    sd = bd.pin_logits(bd.state_dict(h_dim, "default"))
    y, _ = bd.inputs(B, T)
    bits = bd.pinned_bits(B, T)
    assert set(bits.flatten().tolist()) == set(bd.PINNED_BITS)
    noise = bd.pinned_noise(B, T)
    c = bd.pinned_logits_reference(B, T, bits, noise, torch.float64)
    be, bq = bd.logit_tables()
    for v in (0.0, 1e-4, 0.5, 6.9, 6.92, 16.6, 17.4, 25.0, 87.0, 89.0, 104.0, 1e4):
        for b in (be, bq):
            assert (b == np.float32(v)).any() and (b == np.float32(-v)).any()
    assert not torch.equal(be, bq)
    e, q = c["prob"], c["prior"]
    on = lambda p: (p < 1e-3) | (p > 1 - 1e-3)
    assert (on(e) & on(q)).any() and (on(e) & ~on(q)).any() and (~on(e) & on(q)).any() and (~on(e) & ~on(q)).any()
    enc = obv.encode(sd, y, bits, torch.zeros(B, h_dim), dtype=torch.float64)
    assert torch.equal(enc["logit"], be.double()[None, None, :].expand(B, T, 64))
    assert torch.equal(enc["codes"], c["codes"])
    r = torch.tensor([0.1, 0.9, 0.2])
    for noise_, zk in ((None, "z_greedy"), (noise, "z_sampled")):
        f = obv.forward(sd, y, 0.3, noise_ is None, bits, r, noise_, dtype=torch.float64)
        assert torch.equal(f["prob"], e[None, None, :].expand(B, T, 64)) and torch.equal(f["prior"], q[None, None, :].expand(B, T, 64))
        assert torch.equal(f["z"], c[zk])
        assert float((f["kld_frames"] - c["kld_frames"]).abs().max()) < 1e-12 * float(c["kld_frames"].abs().max())
    assert float(c["kld_frames"].max()) > 50                       # the clamp is at work: |log 1e-3| = 6.9 per saturated pair


def test_pinned_gates_closed_form_is_what_the_oracle_computes():
    h_dim, B, T = 128, 5, 3
    sd = bd.pin_gates(bd.state_dict(h_dim, "default"))
    a, c, d, e = bd.gate_tables(h_dim)
    for v in (a, c, d, e):
        assert set(v.tolist()) == set(bd.GATE_GRID)
    assert len({(float(x), float(y)) for x, y in zip(a, c)}) == 49
    assert torch.equal(sd["rnn.bias_ih_l0"][:h_dim] + sd["rnn.bias_hh_l0"][:h_dim], a)
    assert torch.equal(sd["rnn.bias_ih_l0"][h_dim:2 * h_dim] + sd["rnn.bias_hh_l0"][h_dim:2 * h_dim], c)
    h0 = bd.pinned_h0(B, h_dim)
    assert (h0 == 1).any() and (h0 == -1).any() and (h0 == 0).any() and float(h0.abs().max()) == 1.0
    y, bits = bd.inputs(B, T)
    hs = bd.pinned_gates_reference(h0, T, torch.float64)
    enc = obv.encode(sd, y, bits, h0, dtype=torch.float64)
    assert float((enc["all_h"][:, 1] - hs[0]).abs().max()) < 1e-15 and float((enc["h_last"] - hs[2]).abs().max()) < 1e-15
    dec = obv.decode(sd, enc["codes"], h0, dtype=torch.float64)
    assert float((dec["h_last"] - hs[2]).abs().max()) < 1e-15


@pytest.mark.parametrize("M,N,K", bd.ELU_SHAPES)
def test_elu_case_reaches_the_tail(M, N, K):
    pre = bd.elu_case(M, N, K)[3]
    print(f"ELU case {(M, N, K)}: pre-activations in [{float(pre.min()):.1f}, {float(pre.max()):.1f}]")
    assert float(pre.min()) < -25 and float(pre.max()) > 15
