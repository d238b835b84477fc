"""Shared by test_bvrnn_draws_cpu.py and test_gpu_bvrnn_draws.py: the mel coder's weight draws (the default one, which keeps every
logit within 0.5 of zero, a wide one and one that saturates the sigmoids), the pinned checkpoints (one layer's weight zeroed, so that
its pre-activation IS its bias and a whole-model call becomes a unit test of that layer's epilogue against a closed form), the
inputs, the tie rule of free-running comparisons, and the float64 / float32 references (computed once per case and shared).
The elementwise comparison is vocoder_layers.compare."""
import functools

import numpy as np
import torch

import conceal_oracle as co
from bvcodec import config, synth
from oracle import bvrnn as obv
from vocoder_layers import MARGIN, U, Ledger, compare  # noqa: F401  (re-exported: one comparison for the whole suite)

DRAWS = ("default", "wide", "saturated")
GAINS = {"default": None, "wide": (1.7, 8.0, 2.5), "saturated": (2.0, 20.0, 3.0)}     # (g_hidden, g_out, g_gru), synth.bvrnn_state_dict
# free-running cases (h_dim, B, T): a row tile that is not full, a partly filled second one, and 80 rows (the interleaved chains)
SHAPES = ((1024, 20, 48), (256, 20, 48), (128, 5, 48), (1024, 80, 6))
RANGE_HDIMS = (64, 128, 1024)
TEACHER_FRAMES = (0, 1, 7, 23, 47)                      # of the (1024, 20, 48) case
TIE = 1e-5                                              # the project's margin: a rounded argument this close to 0.5 may flip
CAP_SHARE, CAP_ROWS, MIN_FRAMES = 1e-4, 2, 0.9
Z = 64                                                  # the shipped z_dim: the default of everything below that takes a z_dim

# The size classes of tests/test_gpu_coder_sizes.py (profiles/coder_sizes.md): (class, h_dim, z_dim, ((B, T), ...)).  B 5 and 20: a row
# tile that is not full and a partly filled second one; 80 rows x 4 frames: the interleaved chains, which exist at h_dim 1024 only.
SMALL = ((5, 12), (20, 12))
SIZE_CLASSES = (
    ("one k-block", 16, 16, SMALL),
    ("partial waves", 48, 48, SMALL), ("partial waves", 112, 96, SMALL),
    ("Z > H", 64, 128, SMALL),
    ("Z > 3H", 16, 64, SMALL),
    ("table h_dim, other z", 128, 16, SMALL), ("table h_dim, other z", 256, 48, SMALL), ("table h_dim, other z", 512, 96, SMALL),
    ("table h_dim, other z", 1024, 128, ((80, 4),)), ("table h_dim, other z", 1024, 16, SMALL),
    ("no persistent kernel (h_dim)", 192, 64, SMALL), ("no persistent kernel (h_dim)", 384, 32, SMALL), ("no persistent kernel (h_dim)", 1040, 64, SMALL),
    ("no persistent kernel (z_dim)", 64, 144, SMALL),
)
SIZE_DRAWS = ("default", "wide")
SIZE_CASES = tuple((h, z, B, T) for _, h, z, shapes in SIZE_CLASSES for B, T in shapes)
PINNED_SIZES = ((48, 48), (64, 128), (192, 64), (1024, 16))
WIRE_SIZES = ((128, 16), (48, 48), (112, 96), (64, 128))
REJECTED_SIZES = ((24, 64), (1024, 8), (1024, 0), (64, 24))      # h_dim = 24, z_dim = 8, z_dim = 0 (and a z_dim that is no multiple of 16)


def class_of(h_dim, z_dim):
    return next(c for c, h, z, _ in SIZE_CLASSES if (h, z) == (h_dim, z_dim))


# what the library's own size rules say of a model (csrc/k_flow.hip flow_perh, csrc/model.hip build_flow, csrc/recurrence.hip)
def flow_supported(h_dim, z_dim):
    return (h_dim in (128, 256, 512, 1024) or h_dim < 128) and z_dim <= 128


FORWARD_REFUSAL = "bvc_bvrnn_forward: z_dim > h_dim is not supported"
FORWARD_NEEDS_Z = "bvc_bvrnn_forward: pass d_z for this z_dim"
CONCEAL_REFUSAL = "bvc_bvrnn_decode_conceal: z_dim > 3 h_dim is not supported"


def forward_runs(h_dim, z_dim):
    return z_dim <= h_dim


def forward_fallback_runs(h_dim, z_dim, num_mels=80):
    """forward without the caller's z: the sample lives in a workspace buffer (recurrence.hip, run_forward)."""
    return z_dim <= h_dim and (z_dim <= num_mels or 2 * z_dim <= h_dim)


def conceal_runs(h_dim, z_dim):
    return z_dim <= 3 * h_dim


# (h_dim, draw, z_dim) -> checkpoint seed where 1234 does not do: the float32 oracle's OWN rounded outputs break a cap of the tie rule
# there (test_bvrnn_draws_cpu.py / test_coder_sizes_cpu.py hold the reference itself to the caps)
SEEDS = {(256, "wide", 64): 7}


def seed_of(h_dim, draw, z_dim=Z):
    """Checkpoint seed of a case.  1234 everywhere but the entries of SEEDS: at h 256 / z 64 the float32 oracle's own sampled forward
    on the wide draw flips two rounded arguments that lie within 1e-5 of 0.5."""
    return SEEDS.get((h_dim, draw, z_dim), 1234)


def conf_of(h_dim, var_bit=True, z_dim=Z):
    conf = config.load_config(config.DEFAULT_CONFIG if var_bit else config.DEFAULT_CONFIG_64BIT)
    conf["h_dim"] = h_dim
    conf["z_dim"] = z_dim
    return conf


def state_dict(h_dim, draw, var_bit=True, z_dim=Z):
    return synth.bvrnn_state_dict(conf_of(h_dim, var_bit, z_dim), seed_of(h_dim, draw, z_dim), gains=GAINS[draw])


def inputs(B, T, seed=5, z_dim=Z):
    """mel ~ N(-4, 1.6^2), bits per frame integers in 0..z_dim."""
    rng = np.random.default_rng(seed)
    y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32))
    bits = torch.from_numpy(rng.integers(0, z_dim + 1, size=(B, T)).astype(np.float32))
    return y, bits


def bit_mask(bits, z_dim=Z):
    """(B, T, z_dim) bool: position n of a frame carries a bit where bits > n."""
    return bits[:, :, None] > torch.arange(z_dim, dtype=bits.dtype)[None, None, :]


# ---------------------------------------------------------------------------------------------- the tie rule
class Cut:
    """Per row, the first frame at which a rounded value differs from the float64 oracle's (T where none does).  Every differing
    position of that frame must lie within TIE of a tie of the float64 arithmetic; the row is compared up to that frame only."""

    def __init__(self, what, got, ref, arg64, active):
        """got / ref (B, T, Z): rounded values (0 / 1; anything at positions that carry no bit), arg64: the float64 oracle's rounded
        argument, active (B, T, Z) bool: the positions that carry a bit."""
        got, ref, arg64 = (np.asarray(a, dtype=np.float64) for a in (got, ref, arg64))
        active = np.asarray(active, dtype=bool)
        B, T = got.shape[:2]
        differ = (np.abs(got - ref) > 0.25) & active
        assert not (np.abs(got - ref) > 0.25)[~active].any(), f"{what}: a position that carries no bit differs"
        near = (np.abs(arg64 - 0.5) < TIE) & active
        self.what, self.B, self.T = what, B, T
        self.first = np.full(B, T, dtype=np.int64)
        self.excluded, self.compared, self.problems = 0, 0, []
        for b in range(B):
            rows = np.flatnonzero(differ[b].any(axis=1))
            t0 = int(rows[0]) if rows.size else T
            self.first[b] = t0
            self.compared += int(active[b, :t0 + 1].sum())
            if t0 < T:
                bad = differ[b, t0] & ~near[b, t0]
                self.excluded += int(differ[b, t0].sum())
                if bad.any():
                    n = int(np.flatnonzero(bad)[0])
                    self.problems.append(f"{what}: row {b} frame {t0} position {n}: got {got[b, t0, n]!r} expected {ref[b, t0, n]!r}, the float64 "
                                         f"rounded argument is {arg64[b, t0, n]!r} ({int(bad.sum())} such positions in this frame)")
        self.near = int(near.sum())
        self.rows_cut = int((self.first < T).sum())
        self.frames = float(np.minimum(self.first + 1, T).sum()) / (B * T)

    def check(self):
        """The caps of a case: excluded positions at most CAP_SHARE of the compared bits, at most CAP_ROWS rows cut, MIN_FRAMES of the
        frames still compared."""
        assert not self.problems, "\n".join(self.problems[:8])
        assert self.excluded <= CAP_SHARE * self.compared, (self.what, self.excluded, self.compared)
        assert self.rows_cut <= CAP_ROWS, (self.what, self.rows_cut)
        assert self.frames >= MIN_FRAMES, (self.what, self.frames)

    def __str__(self):
        return (f"{self.what}: {self.excluded} differing positions (all within {TIE:g} of a tie) of {self.compared} compared bits, "
                f"{self.near} bits within {TIE:g} of a tie, {self.rows_cut} rows cut, {100 * self.frames:.1f} % of the frames compared")

    def mask(self, a, ref64, inclusive):
        """a (B, T, C) with the frames a row is not compared at replaced by the float64 reference (no error there).  inclusive: the frame
        of the first difference itself still counts (values computed BEFORE the rounding: prob, prior, the state before the frame)."""
        a = n64(a).copy() if torch.is_tensor(a) else np.array(a, dtype=np.float64)
        for b in range(self.B):
            a[b, self.first[b] + (1 if inclusive else 0):] = ref64[b, self.first[b] + (1 if inclusive else 0):]
        return a

    def frames_all_rows(self):
        """Frames before the first cut of any row (for values that are means over the rows)."""
        return int(self.first.min())


def n64(t):
    return t.detach().cpu().to(torch.float64).numpy()


# ---------------------------------------------------------------------------------------------- references of the free-running cases
def reference(draw, h_dim, B, T, z_dim=Z):
    return _reference(draw, h_dim, B, T, z_dim)


@functools.lru_cache(maxsize=None)
def _reference(draw, h_dim, B, T, z_dim):
    """The float64 and float32 oracles on one case: dict of dicts o64 / o32 with encode, decode (of the float64 oracle's codes), forward
    (p_use_gen 0.3, sampled, generator seed 77) and conceal (10 % loss plus a burst per row), the inputs, and the float32 oracle's own
    cuts against the float64 one.  Computed once; nobody changes it."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = state_dict(h_dim, draw, z_dim=z_dim)
    y, bits = inputs(B, T, z_dim=z_dim)
    h0 = torch.zeros(B, h_dim)
    r, noise = obv.draw_randomness(T, B, z_dim, False, generator=torch.Generator().manual_seed(77))
    present = co.loss_pattern(B, T, 0.1, seed=B + T, burst=min(6, T // 3))
    res = dict(sd=sd, y=y, bits=bits, r=r, noise=noise, present=present, mask=bit_mask(bits, z_dim))
    enc64 = obv.encode(sd, y, bits, h0, dtype=torch.float64)
    codes = enc64["codes"].float()
    res["codes"] = codes
    for name, dt in (("o64", torch.float64), ("o32", torch.float32)):
        res[name] = dict(encode=enc64 if name == "o64" else obv.encode(sd, y, bits, h0),
                         decode=obv.decode(sd, codes, h0, dtype=dt),
                         forward=obv.forward(sd, y, 0.3, False, bits, r, noise, dtype=dt),
                         conceal=co.decode_conceal(sd, codes, present, bits, h0, dtype=dt))
    res["cuts32"] = cuts_of(res, res["o32"]["encode"]["codes"], res["o32"]["forward"]["z"], res["o32"]["conceal"]["codes_out"], "float32 oracle")
    return res


def cuts_of(ref, codes, z, codes_out, who, z_dim=None):
    """The three tie cuts of one implementation's rounded outputs against the float64 oracle of `ref` (z_dim: the width `ref` must have)."""
    o = ref["o64"]
    mask = ref["mask"].numpy()
    assert z_dim is None or mask.shape[2] == z_dim == np.shape(codes)[2]
    lost = (~ref["present"])[:, :, None].numpy() & mask
    return dict(encode=Cut(f"{who} encode codes", codes, o["encode"]["codes"], o["encode"]["prob"], mask),
                forward=Cut(f"{who} forward z", z, o["forward"]["z"], o["forward"]["arg"], mask),
                conceal=Cut(f"{who} conceal codes_out", codes_out, o["conceal"]["codes_out"], o["conceal"]["prior"], lost))


def regime(draw, h_dim, B, T, z_dim=Z):
    """What the float64 oracle reaches on a case: the figures of the draws' table."""
    ref = reference(draw, h_dim, B, T, z_dim)
    e64, f64, f32 = ref["o64"]["encode"], ref["o64"]["forward"], ref["o32"]["forward"]
    e, q = f64["prob"], f64["prior"]
    beyond = lambda p: (p < 1e-3) | (p > 1 - 1e-3)
    p32 = torch.cat([f32["prob"], f32["prior"], ref["o32"]["encode"]["prob"]])
    return dict(max_logit=float(e64["logit"].abs().max()), max_h=float(e64["all_h"].abs().max()), max_mel=float(ref["o64"]["decode"]["mel"].abs().max()),
                max_kld=float(f64["kld_frames"].max()), clamp_share=float((beyond(e) | beyond(q)).double().mean()),
                exact01=float(((p32 == 0) | (p32 == 1)).double().mean()))


# ---------------------------------------------------------------------------------------------- pinned logits
LOGIT_TABLE = (0.0, 1e-4, 0.5, 6.9, 6.92, 16.6, 17.4, 25.0, 87.0, 89.0, 104.0, 1e4,      # the clamp at ln 999 = 6.9068, 1 + e^-x == 1, expf overflow
               1e-3, 0.1, 1.0, 2.0, 4.0, 6.0, 6.9068, 8.0, 10.0, 12.0, 15.0, 17.0, 20.0, 30.0, 40.0, 60.0, 80.0, 88.0, 88.7, 100.0)
assert len(LOGIT_TABLE) == 32


def logit_tables(z_dim=Z):
    """(enc.4.bias, prior.4.bias) float32 (z_dim,): the table with both signs (0 twice), in two different orders so that the (e, q)
    pairs cover the KLD clamp on, off and mixed.  z_dim <= 64: the first z_dim entries of the 64-entry tables; beyond 64 the tables
    followed by permutations of themselves (one more per 64 entries), cut at z_dim: the 64 leading values are the same for every z_dim."""
    t = np.array([s * v for v in LOGIT_TABLE for s in (1.0, -1.0)], dtype=np.float32)
    rng = np.random.default_rng(11)
    be, bq = t[rng.permutation(Z)], t[rng.permutation(Z)]
    more = np.random.default_rng(12)
    while be.size < z_dim:
        be, bq = np.concatenate([be, be[:Z][more.permutation(Z)]]), np.concatenate([bq, bq[:Z][more.permutation(Z)]])
    return torch.from_numpy(be[:z_dim].copy()), torch.from_numpy(bq[:z_dim].copy())


def pin_logits(sd):
    sd = dict(sd)
    be, bq = logit_tables(sd["enc.4.bias"].shape[0])
    sd["enc.4.weight"], sd["prior.4.weight"] = torch.zeros_like(sd["enc.4.weight"]), torch.zeros_like(sd["prior.4.weight"])
    sd["enc.4.bias"], sd["prior.4.bias"] = be, bq
    return sd


PINNED_BITS = (0.0, 1.0, 34.5, 63.0, 64.0, 1000.0)      # of the shipped z_dim


def pinned_bit_values(z_dim=Z):
    """No bit, one, a count that is no integer, all but one, all, far more than all.  (0, 1, z/2 + 0.5, z - 1, z, 1000); at 64 the
    fractional count stays the 34.5 the shipped size's tests have always used."""
    return PINNED_BITS if z_dim == Z else (0.0, 1.0, z_dim / 2 + 0.5, z_dim - 1.0, float(z_dim), 1000.0)


def pinned_bits(B, T, z_dim=Z):
    v = pinned_bit_values(z_dim)
    return torch.tensor([[v[(b + 2 * t) % len(v)] for t in range(T)] for b in range(B)], dtype=torch.float32)


def pinned_noise(B, T, seed=3, z_dim=Z):
    """Uniform samples for the sampled forward with every rounded argument u - 0.5 + sigmoid(enc bias) at least 1e-3 from 0.5."""
    Z = z_dim
    e = torch.sigmoid(logit_tables(Z)[0].double())
    u = torch.rand(B, T, Z, generator=torch.Generator().manual_seed(seed))
    d = u.double() - 1.0 + e[None, None, :]
    u = torch.where(d.abs() < 2e-3, torch.where(u < 0.5, u + 4e-3, u - 4e-3), u)
    assert bool(((u.double() - 1.0 + e[None, None, :]).abs() >= 1e-3).all()) and bool((u >= 0).all()) and bool((u < 1).all())
    return u


def pinned_logits_reference(B, T, bits, noise, dtype, z_dim=Z):
    """Closed forms of the pinned-logits checkpoint in `dtype`: prob, prior (Z,), codes (B,T,Z), z greedy / sampled, kld_frames (T,),
    generated (B,T,Z) = masked round(prior).  bits None: a fixed-rate model (no mask)."""
    Z = z_dim
    be, bq = (b.to(dtype) for b in logit_tables(Z))
    e, q = torch.sigmoid(be), torch.sigmoid(bq)
    mask = torch.ones(B, T, Z, dtype=torch.bool) if bits is None else bit_mask(bits, Z)
    half = torch.full((B, T, Z), 0.5, dtype=dtype)
    eb = e[None, None, :].expand(B, T, Z)
    out = dict(prob=e, prior=q, mask=mask)
    out["codes"] = torch.where(mask, torch.round(eb), half)
    out["generated"] = torch.where(mask, torch.round(q)[None, None, :].expand(B, T, Z), half)
    out["z_greedy"] = torch.where(mask, torch.round(eb) - eb + eb, half)
    arg = noise.to(dtype) - 0.5 + eb
    out["arg"] = arg
    out["z_sampled"] = torch.where(mask, torch.round(arg) - eb + eb, half)
    ke = e * (torch.log(torch.clip(e, 1e-3)) - torch.log(torch.clip(q, 1e-3))) + (1 - e) * (torch.log(torch.clip(1 - e, 1e-3)) - torch.log(torch.clip(1 - q, 1e-3)))
    out["kld_frames"] = (ke[None, None, :] * mask.to(dtype)).sum(-1).mean(0)
    return out


# ---------------------------------------------------------------------------------------------- pinned gates
GATE_GRID = (-30.0, -8.0, -1.0, 0.0, 1.0, 8.0, 30.0)


def gate_tables(h_dim):
    """(a, c, d, e) float32 (h_dim,) each from GATE_GRID: b_ir + b_hr, b_iz + b_hz, b_in, b_hn of hidden unit j.  The first 49 units walk
    the (a, c) pairs, every unit draws (d, e) on its own."""
    rng = np.random.default_rng(13)
    g = np.array(GATE_GRID, dtype=np.float32)
    j = np.arange(h_dim)
    return tuple(torch.from_numpy(v) for v in (g[j % 7], g[(j // 7) % 7], g[rng.integers(0, 7, h_dim)], g[rng.integers(0, 7, h_dim)]))


def pin_gates(sd):
    sd = dict(sd)
    H = sd["rnn.weight_hh_l0"].shape[1]
    a, c, d, e = gate_tables(H)
    sd["rnn.weight_ih_l0"], sd["rnn.weight_hh_l0"] = torch.zeros_like(sd["rnn.weight_ih_l0"]), torch.zeros_like(sd["rnn.weight_hh_l0"])
    quarter = torch.full((H,), 0.25)                                   # a - 0.25 and 0.25 are floats, and so is their sum a
    sd["rnn.bias_ih_l0"] = torch.cat([a - quarter, c + quarter, d])
    sd["rnn.bias_hh_l0"] = torch.cat([quarter, -quarter, e])
    return sd


def pinned_h0(B, h_dim, seed=17):
    rng = np.random.default_rng(seed)
    h = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(B, h_dim)).astype(np.float32))
    h[:, 0::7], h[:, 1::7], h[:, 2::7] = 1.0, -1.0, 0.0               # exact +-1 and 0 against every (a, c) pair
    return h


def pinned_gates_reference(h0, steps, dtype):
    """[h_1 ... h_steps] of the pinned-gates checkpoint in `dtype`: r = sigmoid(a), z = sigmoid(c), n = tanh(d + r e), h' = (h - n) z + n."""
    a, c, d, e = (v.to(dtype) for v in gate_tables(h0.shape[1]))
    r, z = torch.sigmoid(a), torch.sigmoid(c)
    n = torch.tanh(d + r * e)
    h, out = h0.to(dtype), []
    for _ in range(steps):
        h = (h - n[None, :]) * z[None, :] + n[None, :]
        out.append(h)
    return out


PINNED = {"logits": pin_logits, "gates": pin_gates}


# ---------------------------------------------------------------------------------------------- one layer deep into the ELU tail
ELU_SHAPES = ((5, 1024, 1024), (20, 1024, 2048), (300, 1024, 80))


@functools.lru_cache(maxsize=None)
def elu_case(M, N, K):
    """x ~ 8 N(0, 1), w ~ N(0, 1 / K), bias ~ -4 + N(0, 1): pre-activations ~ N(-4, 8^2), about [-30, 20] and beyond.
    Returns (x, w, b, pre64, ref64, ref32)."""
    g = torch.Generator().manual_seed(M + N + K)
    x = 8.0 * torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / np.sqrt(K)
    b = -4.0 + torch.randn(N, generator=g)
    pre = torch.nn.functional.linear(x.double(), w.double(), b.double())
    return x, w, b, pre, torch.nn.functional.elu(pre), torch.nn.functional.elu(torch.nn.functional.linear(x, w, b))
