"""CPU checks of tests/conv_ref.py: the dyadic cases are exact in fp32 under any summation order, and they can SEE the defects they are
built for -- an operand that lost its lowest significand bit, a store that truncates, an accumulator kept in fp16 -- which the
small-integer data of the older convolution tests cannot."""
import pytest
import torch
import torch.nn.functional as TF

from tests import conv_ref as R
from tests._helpers import same_bits

# every forward case of tests/test_gpu_conv_pinned.py: the table, the big-tile, first-layer, view and two-source (+ embedding) shapes
FWD = [(s, dt, role, e) for s, e, dts in R.forward_table() for dt in dts for role in R.ROLES]
WGRAD = [(s, dt, role) for s in R.WGRAD_CASES for dt in R.DTYPES for role in R.ROLES]


def _id(v):
    return R.DT_NAME[v] if isinstance(v, torch.dtype) else ("x".join(map(str, v)) if isinstance(v, tuple) else str(v))


def _permuted(c, seed=0):
    perm = torch.randperm(c.shape[1], generator=torch.Generator().manual_seed(seed))
    return c.x[:, perm].contiguous(), c.w[:, perm].contiguous()


@pytest.mark.parametrize("shape,dt,role,emb", FWD, ids=_id)
def test_forward_case_is_exact_in_fp32_in_any_order(shape, dt, role, emb):
    c = R.conv_case(shape, dt, role, emb)
    R.assert_operands(c)
    R.assert_exact(c)
    # fp32 conv2d == float64 conv2d bit for bit, and again with the input channels permuted (another summation order)
    y32 = TF.conv2d(c.x.float(), c.w.float(), c.b.float(), padding=1)
    assert same_bits(y32, c.y.float()) and torch.equal(y32.double(), c.y)
    xp, wp = _permuted(c)
    assert same_bits(TF.conv2d(xp.float(), wp.float(), c.b.float(), padding=1), c.y.float())
    assert torch.equal(TF.conv2d(xp, wp, c.b, padding=1), c.y)
    # the inference epilogue: one fmaf, exact, then the ReLU
    post32 = torch.relu(c.sc.float()[None, :, None, None] * y32 + c.sh.float()[None, :, None, None])
    assert torch.equal(post32.double(), c.post)
    assert bool((c.sc < 0).any()) and bool((c.post == 0).any()) and bool((c.post > 0).any())


@pytest.mark.parametrize("shape,dt,role,emb", FWD, ids=_id)
def test_forward_case_sees_the_defects(shape, dt, role, emb, capsys):
    c = R.conv_case(shape, dt, role, emb)
    want = c.y if dt == R.F32 else R.round_dt(c.y, dt).double()
    got = R.mutant_truncated_operands(c)
    got = got if dt == R.F32 else got.float().to(dt).double()
    assert not torch.equal(got, want), "operands cut to p - 1 bits give the same output"
    if dt == R.F32:
        return
    assert not torch.equal(R.mutant_truncating_store(c.y, dt).double(), want), "a truncating store gives the same output"
    assert not torch.equal(R.mutant_truncating_store(c.post, dt), R.round_dt(c.post, dt)), "a truncating store gives the same activation"
    if dt == R.F16:
        assert not torch.equal(R.mutant_fp16_accumulation(c).double(), want), "fp16 accumulation gives the same output"
    # the store's rounding is exercised: a quarter of the outputs at least are no values of the type (a condition on the INPUTS)
    share = R.rounding_share(c.y, dt)
    with capsys.disabled():
        print(f"\nrounding share {shape} {R.DT_NAME[dt]} {role}: {share:.2f} (plain), {R.rounding_share(c.post, dt):.2f} (inference epilogue)")
    assert share >= 0.25, share
    assert R.rounding_share(c.post, dt) >= 0.25, R.rounding_share(c.post, dt)      # (the ReLU zeroes about half of them: still a quarter)


@pytest.mark.parametrize("shape", R.SLAB_EXACT, ids=_id)
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_slab_case_tells_accumulators_from_rounded_outputs(shape, dt):
    """sum y per channel is exact in fp32 in any order on the slab cases, and differs from the sum of the ROUNDED outputs: a kernel that
    took the statistics from what it stores would be seen."""
    for role in R.ROLES:
        c = R.conv_case(shape, dt, role)
        s1, s2, sa = R.stats_of(c.y)
        assert float(sa.max()) < 2.0 ** 24 * c.q
        assert torch.equal(c.y.float().sum(dim=(0, 2, 3)).double(), s1)
        if dt != R.F32:
            assert not torch.equal(R.round_dt(c.y, dt).double().sum(dim=(0, 2, 3)), s1)


@pytest.mark.parametrize("shape", R.DGRAD_CASES, ids=_id)
@pytest.mark.parametrize("dt", R.DTYPES, ids=_id)
def test_data_gradient_case_is_autograd_s(shape, dt):
    """the data gradient written as a convolution over dy equals autograd's, exactly, in both roles"""
    for role in R.ROLES:
        c, w = R.dgrad_case(shape, dt, role)
        R.assert_operands(c)
        R.assert_exact(c)
        N, Cin, Cout, H, W = shape
        x = torch.zeros((N, Cin, H, W), dtype=torch.float64, requires_grad=True)
        TF.conv2d(x, w, None, padding=1).backward(c.x)
        assert torch.equal(x.grad, c.y_nobias)
        assert same_bits(TF.conv2d(c.x.float(), c.w.float(), None, padding=1), c.y_nobias.float())
        if dt != R.F32:
            assert R.rounding_share(c.y_nobias, dt) >= 0.25
            assert not torch.equal(R.mutant_truncating_store(c.y_nobias, dt), R.round_dt(c.y_nobias, dt))


@pytest.mark.parametrize("shape,dt,role", WGRAD, ids=_id)
def test_weight_gradient_case_is_exact_in_fp32_in_any_order(shape, dt, role):
    c = R.wgrad_case(shape, dt, role)
    N, Cin, Cout, H, W = shape
    assert bool(R.representable(c.x, dt).all()) and bool(R.representable(c.dy, dt).all()) and R.full_share(c.full, c.p) >= 0.5
    assert float(c.absum.max()) < 2.0 ** 24 * c.q
    w32 = torch.zeros((Cout, Cin, 3, 3), requires_grad=True)
    TF.conv2d(c.x.float(), w32, None, padding=1).backward(c.dy.float())
    assert same_bits(w32.grad, c.dw.float()) and torch.equal(w32.grad.double(), c.dw)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1))           # the images in another order: another summation order
    w32p = torch.zeros((Cout, Cin, 3, 3), requires_grad=True)
    TF.conv2d(c.x[perm].flip(3).float(), w32p.flip(3), None, padding=1).backward(c.dy[perm].flip(3).float())
    assert same_bits(w32p.grad, c.dw.float())
    # sensitivity: operands cut to p - 1 significand bits
    cut = torch.nn.grad.conv2d_weight(R.trunc_sig(c.x, c.p - 1), (Cout, Cin, 3, 3), R.trunc_sig(c.dy, c.p - 1), padding=1)
    assert not torch.equal(cut, c.dw)


@pytest.mark.parametrize("dt", (R.BF16, R.F16), ids=_id)
def test_first_layer_cases(dt):
    """12-bit inputs: rounding them to the type differs from truncating them, and the convolution of the rounded input is exact in
    fp32; and of the first-layer cases at least one per role has exact channel sums (the GPU test compares those with ==)."""
    x, xr, w, y = R.first_p12_case(dt)
    assert float((xr != x).double().mean()) > 0.5 and not torch.equal(R.trunc_sig(x, R.SIG_BITS[dt]), xr)
    assert same_bits(TF.conv2d(xr.float(), w.float(), None, padding=1), y.float())
    assert not torch.equal(TF.conv2d(R.trunc_sig(x, R.SIG_BITS[dt]), w, None, padding=1), y)
    assert R.rounding_share(y, dt) >= 0.25 and not torch.equal(R.mutant_truncating_store(y, dt), R.round_dt(y, dt))
    for role in R.ROLES:
        exact = [s for s in R.FIRST_CASES if float(R.stats_of(R.conv_case(s, dt, role).y)[2].max()) < 2.0 ** 24 * R.conv_case(s, dt, role).q]
        assert exact, "no first-layer case with exact channel sums"


def test_case_table_rules():
    """the two launch rules the GPU module states for itself, on the shapes they are about"""
    assert all(R.runs_pair_loop(v, s[1], s[1]) for s, v in R.PAIR_CASES.items())
    assert not R.runs_pair_loop((32, 4, 64, 1), 24, 24) and not R.runs_pair_loop((32, 8, 64, 1), 32, 32) and not R.runs_pair_loop((32, 4, 64, 1), 48, 48)
    assert R.runs_pair_loop((32, 4, 64, 1), 32, 16, ldx1=16, C0=16) and not R.runs_pair_loop((32, 4, 64, 1), 32, 16, ldx1=8, C0=16)
    k16 = [R.wgrad_runs_16x16x32(s[3], s[4]) for s in R.WGRAD_CASES]
    assert True in k16 and False in k16
    assert R.wgrad_runs_16x16x32(40, 64) and not R.wgrad_runs_16x16x32(24, 40) and not R.wgrad_runs_16x16x32(70, 100)


def test_builders_and_mutants_do_what_they_say():
    g = torch.Generator().manual_seed(0)
    for dt in (R.BF16, R.F16):
        p = R.FULL_P[dt]
        v = R.full_operand(g, (4096,), p)
        assert bool(R.representable(v, dt).all()) and R.full_share(v, p) >= 0.55 and float(v.abs().max()) < 2.0
        assert R.quantum(v) == 2.0 ** -(p - 1)
        assert bool((R.trunc_sig(v, p) == v).all()) and bool((R.trunc_sig(v, p - 1).abs() <= v.abs()).all())
        assert float((R.trunc_sig(v, p - 1) != v).double().mean()) >= 0.55
    w = R.pow2_operand(g, (4096,), (-1, 0, 1), 1 / 3)
    assert set(w.tolist()) == {-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0} and R.quantum(w) == 0.5
    assert R.quantum(torch.tensor([0.75, 6.0])) == 0.25 and R.quantum(torch.zeros(3)) == 1.0
    # nearest even against toward zero, on the two sides of a tie in bf16 (8 significand bits: spacing 2 at 256)
    y = torch.tensor([257.0, 258.0, 259.0, -259.0], dtype=torch.float64)
    assert R.round_dt(y, R.BF16).tolist() == [256.0, 258.0, 260.0, -260.0]
    assert R.mutant_truncating_store(y, R.BF16).tolist() == [256.0, 258.0, 258.0, -258.0]
    assert abs(R.gamma(1025) - 1025 * 2.0 ** -24) < 1e-8
