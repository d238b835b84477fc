"""bvc_bvrnn_backward at the row counts of training and at every accepted size (the tables of tests/backward_oracle.py; what each row
case is there for is asserted on the CPU, tests/test_backward_shapes_cpu.py): weight gradients cut into chunks and 128-row blocks,
written as column blocks of a wider gradient through the reduce kernel, bias sums over several blocks, full tiles of the batched GEMM
on the transposed weights, grid-stride loops that run more than once; every row of bvrnn_draws.SIZE_CLASSES, z_dim from 16 to 128;
the saturated draw, where the KLD's clipped formulas run under active bits.  The bar is test_gpu_backward.py's, per gradient tensor:
max|hip - g64| <= 8 x max(e32, 2^-24 max|g64|), e32 the float32 oracle's error with the samples held equal; every case first asserts
that the HIP z equals the oracle's exactly.  Measured ratios: profiles/backward_parity.md.  Needs the MI355X: run with ``-m gpu``."""
import re

import pytest
import torch

import backward_oracle as bo
import bvrnn_draws as bd
from gpu_common import DEV, make_model
from test_gpu_backward import hip_backward, hold

pytestmark = pytest.mark.gpu

LEDGERS = {"rows": bd.Ledger("backward rows"), "saturated": bd.Ledger("backward saturated")}
LEDGERS.update({c: bd.Ledger(f"backward sizes, {c}") for c in dict.fromkeys(bd.class_of(h, z) for h, z in bo.SIZES)})


def model_of(case):
    model, _, sd, _ = make_model(var_bit=case[2], h_dim=case[0], gains=bd.GAINS[case[1]], z_dim=bo.z_of(case))
    return model, sd


def against_oracle(case, ledger):
    """One backward call of a selected case: z exact, every gradient (the input's too) to the bar.  Returns (model, case inputs, forward)."""
    model, sd = model_of(case)
    c = bo.select(case, sd)
    got, fwd = hip_backward(model, c)
    assert torch.equal(fwd["z"].cpu().double(), c["f64"]["z"]), "the samples differ from the oracle's"
    g32, _ = bo.grads(sd, c["y"], c["bits"], c["p_use_gen"], c["greedy"], c["r"], c["noise"], c["gdec"], c["gkld"], torch.float32,
                      z=c["f64"]["z"], var_bit=case[2])
    assert set(got) == set(c["g64"]) and all(got[k].shape == c["g64"][k].shape for k in got)
    hold(got, c["g64"], g32, bo.case_id(case), ledger)
    return model, c, fwd


@pytest.mark.parametrize("case", bo.ROW_CASES, ids=bo.case_id)
def test_backward_at_training_row_counts(case):
    against_oracle(case, LEDGERS["rows"])


@pytest.mark.parametrize("case", bo.SIZE_CASES, ids=bo.case_id)
def test_backward_at_accepted_sizes(case):
    """Also: the forward outputs of the call are bvc_bvrnn_forward's bits at this size.  (112, 96): forward refuses to run without
    the caller's z; the backward pass hands its own over and runs."""
    model, c, fwd = against_oracle(case, LEDGERS[bd.class_of(case[0], case[7])])
    dec, kld, ex = model.bvrnn.forward(c["y"].to(DEV), c["p_use_gen"], c["greedy"], c["bits"].to(DEV), r=c["r"], noise=c["noise"], return_all=True)
    assert torch.equal(fwd["dec"], dec) and torch.equal(fwd["kld"], kld)
    for k in ("z", "prob", "prior", "kld_frames"):
        assert torch.equal(fwd[k], ex[k]), k


@pytest.mark.parametrize("case", bo.SATURATED_CASES, ids=bo.case_id)
def test_backward_on_the_saturated_draw(case):
    """e, 1 - e, prior and 1 - prior below the KLD's clip of 1e-3 under active bits (counted on the CPU): code_bwd_kernel's clipped
    formulas against autograd of the reference's own expression."""
    _, c, fwd = against_oracle(case, LEDGERS["saturated"])
    act = (torch.arange(bo.z_of(case))[None, None, :] < c["bits"][:, :, None])
    assert bool((fwd["prob"].cpu()[act] < bo.CLIP).any()) and bool((fwd["prior"].cpu()[act] < bo.CLIP).any())


@pytest.mark.parametrize("h_dim,z_dim", bo.REFUSED_SIZES)
def test_backward_refuses_what_forward_refuses(h_dim, z_dim):
    """z_dim > h_dim: the forward's refusal, before anything is launched (the gradient buffer is untouched), and the model still
    encodes the same bits.  Every buffer is sized from the model's own configuration."""
    from bvcodec import _abi
    model = make_model(True, h_dim, z_dim=z_dim)[0]
    B, T = 5, 12
    y, bits = bd.inputs(B, T, z_dim=z_dim)
    y, bits = y.to(DEV), bits.to(DEV)
    h0 = torch.zeros(1, B, h_dim, device=DEV)
    before = model.bvrnn.encode(y, bits, h0)[0].clone()
    with pytest.raises(RuntimeError, match=re.escape(bd.FORWARD_REFUSAL)):
        model.bvrnn.backward(y, 0.5, True, bits, torch.ones(B, T, 80, device=DEV), 1.0)
    eng = model.bvrnn.engine(y)
    total = model.bvrnn.grad_layout()[1]
    flat = torch.full((total,), 777.0, device=DEV)
    gdec = torch.ones(B, T, 80, device=DEV)
    use = torch.zeros(T, dtype=torch.uint8)
    need = int(eng.lib.bvc_bvrnn_backward_workspace_bytes(eng.handle, B, T))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = eng.lib.bvc_bvrnn_backward(eng.handle, _abi.ptr(y), _abi.ptr(bits), _abi.ptr(use, torch.uint8), 1, 0, None, B, T, _abi.ptr(gdec), 1.0,
                                    _abi.ptr(flat), None, None, None, None, None, None, _abi.ptr(ws, torch.uint8), need, eng.stream())
    assert rc == -1 and bd.FORWARD_REFUSAL.encode() in eng.lib.bvc_last_error()                # BVC_EINVAL
    torch.cuda.synchronize()
    assert bool((flat == 777.0).all()), "a refused call wrote gradients"
    assert torch.equal(model.bvrnn.encode(y, bits, h0)[0], before)
    model.check_status()


def test_backward_shapes_ledger():
    """Prints the PARITY lines of the new families (profiles/backward_parity.md)."""
    for led in LEDGERS.values():
        led.close()
