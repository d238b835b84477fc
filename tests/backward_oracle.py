"""Oracle of the backward pass of ``BVRNN.forward`` (bvrnn.py:86-160): the forward restated so that torch.autograd differentiates it
as it differentiates the reference (test infrastructure).

``oracle.bvrnn.forward`` cannot serve: it runs under no_grad and writes the straight-through sample as ``round(arg) - e + e``, whose
derivative is zero.  The reference detaches (bvrnn.py:124,126): ``round(arg(e.detach())) - e.detach() + e``, so the sample's forward
value is the rounded one and its derivative with respect to enc_t is one.  Everything else is the reference's own graph: the clips of
the KLD pass a gradient where torch.clip does, h and h2 run as two chains of the same GRU weights, the frame's networks read the
state ``r[t] < p_use_gen`` selects.  The layers are oracle.bvrnn's (they carry no no_grad).

At float32 the gradients are the reference's bit for bit (tests/golden/make_golden_backward.py asserts it when it writes the g13
fixtures, tests/test_backward_cpu.py holds the stored ones to the project's bar)."""
import torch

from oracle import bvrnn as obv

NOT_TRAINED = ("mean_mel", "std_mel", "log_sigma")       # buffers, and the loss's own scale (not in forward: bvrnn.py:86-160)


def trainable(sd):
    """The names ``BVRNN.forward`` has a gradient for, in state-dict order."""
    return [k for k in sd if k not in NOT_TRAINED]


def forward(sd, y, bits, p_use_gen, greedy, r, noise, var_bit=True, z=None, ste=None):
    """The differentiable pass on tensors of one dtype (``sd`` and ``y`` may require grad).  z (B,T,Z): the samples' forward values
    from another run, used instead of this run's own rounding (float32 against float64 with the samples held equal).  ste (B,T,Z):
    the sample is ``ste + e`` - with ste = round(arg) - e of a base point this is a smooth function whose true derivative there is
    the straight-through one, which is what central differences can be taken of.
    Returns dict(dec (B,T,X), kld scalar, z, prob, prior, arg (B,T,Z))."""
    dtype = y.dtype
    mean, std = sd["mean_mel"], sd["std_mel"]
    px = obv.phi_x(sd, (y - mean[None, None, :]) / std[None, None, :])                       # bvrnn.py:95-100
    B, T = y.shape[:2]
    H = sd["rnn.weight_hh_l0"].shape[1]
    zdim = sd["enc.4.weight"].shape[0]
    h = torch.zeros(B, H, dtype=dtype)
    h2 = torch.zeros(B, H, dtype=dtype)
    mask = None
    if var_bit:
        mask = (torch.as_tensor(bits).to(dtype)[:, :, None] > torch.arange(zdim, dtype=dtype)[None, None, :]).to(dtype)
    outs = dict(dec=[], z=[], prob=[], prior=[], arg=[])
    kld = []
    for t in range(T):
        hs = h2 if bool(r[t] < p_use_gen) else h                                              # bvrnn.py:115-120
        e = torch.sigmoid(obv.enc_logits(sd, torch.cat([px[:, t], hs], 1)))
        pr = obv.prior_prob(sd, hs)
        ed = e.detach()
        arg = ed if greedy else torch.as_tensor(noise[:, t]).to(dtype) - 0.5 + ed             # bvrnn.py:124,126
        if ste is not None:
            zt = torch.as_tensor(ste[:, t]).to(dtype) + e
        else:
            zt = (torch.round(arg) if z is None else torch.as_tensor(z[:, t]).to(dtype)) - ed + e
        if var_bit:                                                                           # bvrnn.py:128-129
            zt = zt * mask[:, t] + 0.5 * (1 - mask[:, t])
        pz = obv.phi_z(sd, zt)
        d = obv.dec(sd, torch.cat([pz, hs], 1))                                               # bvrnn.py:134-137
        pxg = obv.phi_x(sd, (d - mean[None, :]) / std[None, :])                               # bvrnn.py:139
        if p_use_gen < 1:                                                                     # bvrnn.py:142-145
            h = obv.gru_cell(sd, torch.cat([px[:, t], pz], 1), h)
        if p_use_gen > 0:
            h2 = obv.gru_cell(sd, torch.cat([pxg, pz], 1), h2)
        ke = e * (torch.log(torch.clip(e, 1e-3)) - torch.log(torch.clip(pr, 1e-3))) + \
            (1 - e) * (torch.log(torch.clip(1 - e, 1e-3)) - torch.log(torch.clip(1 - pr, 1e-3)))      # bvrnn.py:148-149
        kld.append(torch.mean(torch.sum(ke * mask[:, t] if var_bit else ke, -1)))
        for k, v in (("dec", d), ("z", zt), ("prob", e), ("prior", pr), ("arg", arg)):
            outs[k].append(v)
    res = {k: torch.stack(v).permute(1, 0, 2) for k, v in outs.items()}
    res["kld"] = torch.mean(torch.stack(kld))                                                 # bvrnn.py:160
    return res


def grads(sd, y, bits, p_use_gen, greedy, r, noise, gdec, gkld, dtype, z=None, var_bit=True):
    """The vector-Jacobian product at (gdec (B,T,X), gkld scalar), computed at ``dtype``.  Returns (g, fwd): g maps every trainable
    name to its gradient (zeros where the pass does not reach a tensor) and "y" to the input's; fwd holds the detached dec, kld, z,
    prob, prior and arg of that run."""
    p = {k: torch.as_tensor(v).to(dtype).clone() for k, v in sd.items() if k != "log_sigma"}
    names = trainable(p)
    for k in names:
        p[k].requires_grad_(True)
    yl = torch.as_tensor(y).to(dtype).clone().requires_grad_(True)
    out = forward(p, yl, bits, p_use_gen, greedy, r, noise, var_bit=var_bit, z=z)
    loss = (out["dec"] * torch.as_tensor(gdec).to(dtype)).sum() + out["kld"] * float(gkld)
    got = torch.autograd.grad(loss, [p[k] for k in names] + [yl], allow_unused=True)
    g = {k: (torch.zeros_like(p[k]) if v is None else v) for k, v in zip(names, got[:-1])}
    g["y"] = torch.zeros_like(yl) if got[-1] is None else got[-1]
    return g, {k: v.detach() for k, v in out.items()}


# ---------------------------------------------------------------------------------------------- case selection
ROUND_MARGIN = 2e-5          # twice the project's tie width (bvrnn_draws.TIE); the forward's measured probability error is 1.2e-7
CLIP_MARGIN, CLIP = 1e-5, 1e-3
N_ENTRIES, ENTRY_SEED = 4096, 13
MODES = ((0.0, True), (1.0, False), (0.5, False), (0.5, True))        # (p_use_gen, greedy) of tests/golden/make_golden_forward.py


def margins(f64, bits, zdim):
    """Of a float64 run: (distance of the rounded arguments of active bits from 0.5, distance of e, 1 - e, prior, 1 - prior under the
    mask from the clip of the KLD).  bits None: a fixed-rate model, every bit active."""
    B, T = f64["arg"].shape[:2]
    act = torch.ones(B, T, zdim, dtype=torch.bool) if bits is None else torch.arange(zdim)[None, None, :] < bits[:, :, None]
    if not bool(act.any()):
        return float("inf"), float("inf")
    rm = float((f64["arg"] - 0.5).abs()[act].min())
    e, q = f64["prob"][act], f64["prior"][act]
    cm = float(torch.stack([(v - CLIP).abs().min() for v in (e, 1 - e, q, 1 - q)]).min())
    return rm, cm


def entries(numel):
    """The entries of a weight matrix of ``numel`` elements that the h_dim 1024 fixture stores (flat indices, ascending)."""
    import numpy as np
    if numel <= N_ENTRIES:
        return np.arange(numel)
    return np.sort(np.random.default_rng(ENTRY_SEED + numel).choice(numel, N_ENTRIES, replace=False))


def _cases():
    """(h_dim, draw, var_bit, B, T, mode, bits): bits "random" or a count for every frame.  h_dim 64 takes the whole (B, T, mode) grid -
    both sides of the 16-row padding, one frame (no carry), two (one carry), seven (frames switch chains) - and the other axes one at a
    time; h_dim 1024 the (B, T) grid at the mode with both chains and the other axes one at a time; 256 and 512 one case each."""
    out = [(64, "default", True, B, T, m, "random") for B in (1, 3, 17) for T in (1, 2, 7) for m in range(4)]
    out += [(64, "default", False, 3, 7, m, "random") for m in range(4)] + [(64, "wide", True, 3, 7, m, "random") for m in range(4)]
    out += [(64, "default", True, 3, 7, 2, n) for n in (0, 35, 64)]
    out += [(1024, "default", True, B, T, 2, "random") for B in (1, 3, 17) for T in (1, 2, 7)]
    out += [(1024, "default", True, 3, 7, m, "random") for m in (0, 1, 3)]
    out += [(1024, "default", False, 3, 7, 2, "random"), (1024, "wide", True, 3, 7, 2, "random"), (1024, "wide", True, 17, 2, 1, "random"),
            (1024, "default", True, 3, 2, 2, 0), (1024, "default", True, 3, 2, 2, 64), (1024, "default", True, 3, 2, 2, 35)]
    out += [(256, "default", True, 3, 7, 2, "random"), (512, "default", True, 3, 7, 2, "random")]
    return tuple(out)


CASES = _cases()

# ---- the cases of tests/test_gpu_backward_shapes.py: the same tuple, with a z_dim behind it where that is not 64, and "uptoN" for
# bits drawn from 0..N.  Which path of the pass each ROW_CASES entry is there for: paths() below, asserted in test_backward_shapes_cpu.py.
ROW_CASES = (
    (64, "default", True, 5, 48, 2, "random"),        # 240 rows: one chunk of two blocks, the second short; the carries cross 48 frames
    (64, "default", True, 17, 16, 2, "random"),       # 272 rows, 544 stacked: enc.0 / dec.0 / weight_ih in chunks with ldo = 2 K
    (64, "default", True, 17, 16, 0, "upto8"),        # only chain h ran: Mg = TB (greedy: every e is the rounded argument, so few bits)
    (256, "default", True, 17, 16, 1, "random"),      # only chain h2 ran: Mg = TB from row TB on; full tiles of the batched GEMM
    (1024, "default", True, 17, 16, 2, "random"),     # H x H in two chunks, 3H x H one chunk of three blocks
    (1040, "default", True, 17, 16, 2, "random"),     # N K > 4096 x 256 in chunks: the reduce kernel loops
    (1024, "default", True, 66, 16, 2, 8),            # TB H > 4096 x 256: the all-frame kernels loop
)
SIZES = ((16, 16), (48, 48), (112, 96), (128, 16), (256, 48), (512, 96), (1024, 128), (1024, 16), (192, 64), (384, 32), (1040, 64))
REFUSED_SIZES = ((64, 128), (16, 64), (64, 144))      # z_dim > h_dim: the forward's refusal
SIZE_SHAPES = {(1024, 128): ((80, 4),)}                # every other size: bvrnn_draws.SMALL
SIZE_CASES = tuple((h, draw, True, B, T, 2, "random", z) for h, z in SIZES for B, T in SIZE_SHAPES.get((h, z), ((5, 12), (20, 12)))
                   for draw in ("default", "wide"))
SATURATED_CASES = ((64, "saturated", True, 3, 7, 2, "random"), (64, "saturated", True, 3, 7, 3, "random"),
                   (64, "saturated", True, 17, 7, 1, "upto8"), (1024, "saturated", True, 3, 7, 2, "random"))
TRAINING_ROWS = 32 * 344                               # profiles/backward_cost.md


def z_of(case):
    return case[7] if len(case) > 7 else 64


def case_id(c):
    return f"h{c[0]}-{c[1]}-{'var' if c[2] else 'fix'}-B{c[3]}-T{c[4]}-m{c[5]}-bits{c[6]}" + (f"-z{c[7]}" if len(c) > 7 else "")


def draw_inputs(case, seed, z_dim=None):
    """The inputs of a case at one seed: dict(y, bits, r, noise, gdec, gkld, p_use_gen, greedy).  z_dim: the case's own (z_of)."""
    import numpy as np
    h_dim, draw, var_bit, B, T, mode, nbits = case[:7]
    z_dim = z_of(case) if z_dim is None else z_dim
    p_use_gen, greedy = MODES[mode]
    rng = np.random.default_rng(seed)
    y = torch.from_numpy((-4.0 + 1.6 * rng.standard_normal((B, T, 80))).astype(np.float32))
    bits = torch.from_numpy(rng.integers(0, z_dim + 1, size=(B, T)).astype(np.float32))
    if isinstance(nbits, str) and nbits.startswith("upto"):
        bits = torch.remainder(bits, float(int(nbits[4:]) + 1))
    elif nbits != "random":
        bits = torch.full((B, T), float(nbits))
    r = torch.from_numpy(rng.random(T).astype(np.float32))
    noise = None if greedy else torch.from_numpy(rng.random((B, T, z_dim)).astype(np.float32))
    gdec = torch.from_numpy(rng.standard_normal((B, T, 80)).astype(np.float32))
    return dict(y=y, bits=bits, r=r, noise=noise, gdec=gdec, gkld=0.5 + float(rng.random()), p_use_gen=p_use_gen, greedy=greedy)


_FOUND, _SELECTED = {}, {}
SEARCHED = {"forwards": 0, "gradients": 0}             # what the search has computed so far (test_backward_shapes_cpu.py)


def find_seed(case, sd, z_dim=None):
    """The first seed (from a base that depends on the case) at which the float64 forward keeps the margins: dict(inputs.., seed, f64,
    margins).  Searched, never skipped: a case without such a seed among 200 is an error.  No gradient is taken.  Cached."""
    z_dim = z_of(case) if z_dim is None else z_dim
    if (case, z_dim) in _FOUND:
        return _FOUND[(case, z_dim)]
    import zlib
    var_bit = case[2]
    assert sd["enc.4.weight"].shape[0] == z_dim, (case_id(case), sd["enc.4.weight"].shape[0], z_dim)
    p64 = {k: torch.as_tensor(v).double() for k, v in sd.items() if k != "log_sigma"}
    base = zlib.crc32(case_id(case).encode()) % 100000
    for seed in range(base, base + 200):
        inp = draw_inputs(case, seed, z_dim)
        with torch.no_grad():
            f64 = forward(p64, inp["y"].double(), inp["bits"], inp["p_use_gen"], inp["greedy"], inp["r"], inp["noise"], var_bit=var_bit)
        SEARCHED["forwards"] += 1
        rm, cm = margins(f64, inp["bits"] if var_bit else None, z_dim)
        if rm >= ROUND_MARGIN and cm >= CLIP_MARGIN:
            _FOUND[(case, z_dim)] = dict(inp, seed=seed, tried=seed - base + 1, f64=f64, margins=(rm, cm))
            return _FOUND[(case, z_dim)]
    raise AssertionError(f"{case_id(case)}: no seed in [{base}, {base + 200}) keeps the margins")


def select(case, sd, z_dim=None):
    """find_seed's case with the float64 gradients g64, taken once, at the seed found (f64: that run's forward, the same values).  Cached."""
    z_dim = z_of(case) if z_dim is None else z_dim
    if (case, z_dim) not in _SELECTED:
        c = find_seed(case, sd, z_dim)
        g64, f64 = grads(sd, c["y"], c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], c["gdec"], c["gkld"], torch.float64, var_bit=case[2])
        SEARCHED["gradients"] += 1
        assert margins(f64, c["bits"] if case[2] else None, z_dim) == c["margins"]
        _SELECTED[(case, z_dim)] = dict(c, g64=g64, f64=f64)
    return _SELECTED[(case, z_dim)]


# ---------------------------------------------------------------------------------------------- which code a case runs
# Restated from csrc/k_backward.hip (weight_grad_cut, blocks_for), csrc/backward.hip (run_backward's launches, carve_backward's b.wg) and
# csrc/k_gemm_batched.hip (the LDS path and its tile heights), so that a change of a rule is a change of this file too.
TILE, BLOCK, MIN_CHUNK, TARGET = 64, 128, 256, 512
GRID_ELEMENTS = 4096 * 256                             # what one trip of a grid-stride loop covers
LDS_HEIGHTS = (144, 128, 112)


def want_cut(M, N, K):
    """(chunks, rows per chunk) of a weight gradient."""
    tiles = -(-N // TILE) * -(-K // TILE)
    want = max(1, min(-(-TARGET // tiles), -(-M // MIN_CHUNK)))
    rows = -(-(-(-M // want)) // BLOCK) * BLOCK
    return -(-M // rows), rows


def ws_floats(M, N, K):
    chunks, _ = want_cut(M, N, K)
    return chunks * N * K if chunks > 1 else 0


def wg_floats(H, X=80):
    """The floats of the chunk-sum workspace b.wg."""
    return 512 * 4096 + 6 * H * H + 3 * H * X


def weight_grads(H, Z, B, T, mode, X=80):
    """[(name, M, N, K, ldo)] of every launch_weight_grad of one call, and [(name, M, N)] of every launch_col_sum."""
    p_use_gen = MODES[mode][0]
    M1 = B * T
    Mp = 2 * M1 if p_use_gen > 0 else M1
    Mg = (M1 if p_use_gen < 1 else 0) + (M1 if p_use_gen > 0 else 0)
    w = [("phi_x.0", Mp, H, X, X), ("phi_x.2", Mp, H, H, H), ("phi_x.4", Mp, H, H, H),
         ("phi_z.0", M1, H, Z, Z), ("phi_z.2", M1, H, H, H), ("phi_z.4", M1, H, H, H),
         ("enc.0[:, :H]", M1, H, H, 2 * H), ("enc.0[:, H:]", M1, H, H, 2 * H), ("enc.2", M1, H, H, H), ("enc.4", M1, Z, H, H),
         ("prior.0", M1, H, H, H), ("prior.2", M1, H, H, H), ("prior.4", M1, Z, H, H),
         ("dec.0[:, :H]", M1, H, H, 2 * H), ("dec.0[:, H:]", M1, H, H, 2 * H), ("dec.2", M1, H, H, H), ("dec.4", M1, H, H, H),
         ("dec.6", M1, X, H, H),
         ("weight_ih[:, :H]", Mg, 3 * H, H, 2 * H), ("weight_ih[:, H:]", Mg, 3 * H, H, 2 * H), ("weight_hh", Mg, 3 * H, H, H)]
    b = [(n, Mp, H) for n in ("phi_x.0", "phi_x.2", "phi_x.4")] + [(n, M1, H) for n in ("phi_z.0", "phi_z.2", "phi_z.4", "enc.0", "enc.2",
         "prior.0", "prior.2", "dec.0", "dec.2", "dec.4")] + [("enc.4", M1, Z), ("prior.4", M1, Z), ("dec.6", M1, X), ("bias_ih", Mg, 3 * H),
                                                                ("bias_hh", Mg, 3 * H)]
    return w, b


PATHS = ("seam", "chunks ldo == K", "chunks ldo != K enc.0", "chunks ldo != K dec.0", "chunks ldo != K weight_ih[:, :H]",
         "chunks ldo != K weight_ih[:, H:]", "short last chunk", "col_sum blocks", "batched GEMM full tile + tail", "all-frame loop",
         "reduce loop")


def paths(case):
    """The subset of PATHS that one call of the case runs."""
    H, B, T, mode = case[0], case[3], case[4], case[5]
    TB = B * T
    w, b = weight_grads(H, z_of(case), B, T, mode)
    out = set()
    for name, M, N, K, ldo in w:
        chunks, rows = want_cut(M, N, K)
        if chunks == 1 and M > BLOCK and M % BLOCK:
            out.add("seam")                                     # tot += acc after 128 rows, then a short block
        if chunks > 1:
            half = name if name.startswith("weight_ih") else name.split("[")[0]
            out.add("chunks ldo == K" if ldo == K else "chunks ldo != K " + half)
            if M % rows:
                out.add("short last chunk")
            if N * K > GRID_ELEMENTS:
                out.add("reduce loop")
    if any(M > BLOCK for _, M, _ in b):
        out.add("col_sum blocks")
    # d phi_x through the transposed phi_x.4 / .2 (N = K = H) on the LDS kernels: a full tile at whichever height the cut takes, and rows left over
    if H % 256 == 0 and TB > max(LDS_HEIGHTS) and all(TB % h for h in LDS_HEIGHTS):
        out.add("batched GEMM full tile + tail")
    if TB * H > GRID_ELEMENTS:
        out.add("all-frame loop")                               # elu_bwd over dP, unpack_frames of the tape
    return out
