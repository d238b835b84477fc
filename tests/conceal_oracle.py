"""The concealing decoder (``bvc_bvrnn_decode_conceal``, include/bvcodec.h) composed from the CPU oracle's own pieces
(oracle/bvrnn.py: ``prior_prob``, ``phi_z``, ``dec``, ``phi_x``, ``gru_cell``); test infrastructure, float32 or float64.

Per row with state h_t (h_0 = ``h0``), frame t:
    p_t = prior(h_t)                                      bvrnn.py:68-73, sigmoid included
    g_t = round-half-even(p_t), 0.5 at positions >= bits[b, t] on a var_bit model   (bvrnn.py:193-194)
    z_t = codes[b, t] if present[b, t] else g_t           a select: lost positions of ``codes`` are never used
    phi_z, dec, phi_x((dec - mean) / std), GRU            bvrnn.py:223-227
"""
import torch

from oracle import bvrnn as obv


@torch.no_grad()
def decode_conceal(sd, codes, present, bits, h0, var_bit=True, dtype=torch.float32, mode="prior"):
    """codes (B,T,Z), present (B,T) bool, bits (B,T) or None, h0 (B,H).  mode "prior": the operator above; "none": a lost
    frame is a frame of no bits (all 0.5), what a receive session does without concealment.

    Returns dict(mel (B,T,X), h_last (B,H), codes_out (B,T,Z) = z_t, prior (B,T,Z) = p_t of every frame)."""
    sd = obv.cast_state(sd, dtype)
    codes = torch.as_tensor(codes).to(dtype)
    present = torch.as_tensor(present).bool()
    h = torch.as_tensor(h0).to(dtype)
    mean, std = sd["mean_mel"], sd["std_mel"]
    B, T, Z = codes.shape
    if var_bit:
        b = torch.as_tensor(bits).to(dtype)
        mask = b[:, :, None] > torch.arange(Z, dtype=dtype)[None, None, :]
    mel, zs, ps = [], [], []
    for t in range(T):
        p = obv.prior_prob(sd, h)
        g = torch.round(p)
        if var_bit:
            g = torch.where(mask[:, t], g, torch.full_like(g, 0.5))
        if mode == "none":
            g = torch.full_like(g, 0.5)
        z = torch.where(present[:, t, None], codes[:, t], g)
        pz = obv.phi_z(sd, z)
        d = obv.dec(sd, torch.cat([pz, h], 1))
        pxg = obv.phi_x(sd, (d - mean[None, :]) / std[None, :])
        h = obv.gru_cell(sd, torch.cat([pxg, pz], 1), h)
        mel.append(d); zs.append(z); ps.append(p)
    st = lambda l: torch.stack(l).permute(1, 0, 2).contiguous()
    return dict(mel=st(mel), h_last=h, codes_out=st(zs), prior=st(ps))


@torch.no_grad()
def decode_with_prior(sd, codes_out, h0, dtype=torch.float32):
    """``oracle.bvrnn.decode(codes_out)`` that also returns p_t = prior(h_t) at every state it visits (the states follow from the
    filled codes alone): dict(mel (B,T,X), h_last (B,H), prior (B,T,Z))."""
    sd = obv.cast_state(sd, dtype)
    z = torch.as_tensor(codes_out).to(dtype)
    h = torch.as_tensor(h0).to(dtype)
    mean, std = sd["mean_mel"], sd["std_mel"]
    mel, ps = [], []
    for t in range(z.shape[1]):
        ps.append(obv.prior_prob(sd, h))
        pz = obv.phi_z(sd, z[:, t])
        d = obv.dec(sd, torch.cat([pz, h], 1))
        pxg = obv.phi_x(sd, (d - mean[None, :]) / std[None, :])
        h = obv.gru_cell(sd, torch.cat([pxg, pz], 1), h)
        mel.append(d)
    st = lambda l: torch.stack(l).permute(1, 0, 2).contiguous()
    return dict(mel=st(mel), h_last=h, prior=st(ps))


def prior_at_states(sd, codes_out, h0, dtype=torch.float32):
    return decode_with_prior(sd, codes_out, h0, dtype)["prior"]


def loss_pattern(B, T, rate, seed, burst=10, all_lost_row=None, clean_row=None):
    """present (B,T) bool: `rate` random loss, one burst of `burst` frames per row at a row-specific place, optionally one row all
    lost and one row without loss."""
    g = torch.Generator().manual_seed(seed)
    present = torch.rand(B, T, generator=g) >= rate
    for b in range(B):
        if T > burst + 2:
            s = int(torch.randint(1, T - burst, (1,), generator=g))
            present[b, s:s + burst] = False
    if all_lost_row is not None:
        present[all_lost_row] = False
    if clean_row is not None:
        present[clean_row] = True
    return present
