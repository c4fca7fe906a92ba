"""CPU-only checks of tests/temporal_ref.py, the references tests/test_gpu_temporal.py holds the embedding-branch kernels against:
the explicit LSTM loop against torch's nn.LSTM and a hand-stepped nn.LSTMCell in float64, against the recorded numbers of the original
project (g11_temporal_828.npz), and the Linear / metadata-MLP references against torch's own operators.  No kernel is launched here."""
import pytest
import torch

from tests import temporal_ref as TR
from tests._helpers import load_npz, rel_err, sub, t

F64 = torch.float64
LSTM_CASES = [(2, 1, 1), (3, 9, 5), (2, 17, 33), (1, 41, 128)]


def _rel(a, b):
    """max |a - b| / max |b|; two exact zeros agree"""
    return TR.yardstick(b, a)


@pytest.mark.parametrize("B,T,H", LSTM_CASES, ids=["x".join(map(str, c)) for c in LSTM_CASES])
def test_lstm_ref_equals_nn_lstm_in_float64(B, T, H):
    """h_T and all four parameter gradients for a random dh_last against nn.LSTM(1, H, batch_first=True).double(): two float64
    evaluations of one formula, 1e-12 relative.  The per-step gates and cells against a second spelling, nn.LSTMCell stepped by hand."""
    c = TR.lstm_case(B, T, H, seed=100 * H + T)
    ref = TR.lstm_ref_all(c["x"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"], c["dh_last"], F64)
    assert ref["gates"].shape == (B, T, 4 * H) and ref["cells"].shape == (B, T, H) and ref["h_last"].shape == (B, H)
    assert ref["gates"].dtype == F64 and ref["dw_hh"].shape == (4 * H, H) and ref["dw_ih"].shape == (4 * H,)
    lstm = torch.nn.LSTM(1, H, batch_first=True).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(c["w_ih"].double().view(4 * H, 1))
        lstm.weight_hh_l0.copy_(c["w_hh"].double())
        lstm.bias_ih_l0.copy_(c["b_ih"].double())
        lstm.bias_hh_l0.copy_(c["b_hh"].double())
    _, (hn, _) = lstm(c["x"].double().unsqueeze(-1))
    assert _rel(ref["h_last"], hn[-1].detach()) <= 1e-12
    hn[-1].backward(c["dh_last"].double())
    for k, p in (("dw_ih", lstm.weight_ih_l0), ("dw_hh", lstm.weight_hh_l0), ("db_ih", lstm.bias_ih_l0), ("db_hh", lstm.bias_hh_l0)):
        assert _rel(ref[k], p.grad.reshape(ref[k].shape)) <= 1e-12, k
    if T == 1:
        assert float(ref["dw_hh"].abs().max()) == 0.0          # h_0 = 0: the recurrent weights have no gradient after one step
    assert torch.equal(ref["db_ih"], ref["db_hh"])

    cell = torch.nn.LSTMCell(1, H).double()
    with torch.no_grad():
        for dst, src in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)):
            dst.copy_(src)
        h, cc = torch.zeros(B, H, dtype=F64), torch.zeros(B, H, dtype=F64)
        for s in range(T):
            h_prev, c_prev = h, cc
            h, cc = cell(c["x"][:, s, None].double(), (h_prev, c_prev))
            assert _rel(ref["cells"][:, s], cc) <= 1e-12, s
            i, f, g, o = ref["gates"][:, s].split(H, dim=1)
            # the four gates of the step tie the cell's (h, c) to the previous ones
            assert _rel(f * c_prev + i * g, cc) <= 1e-12 and _rel(o * torch.tanh(cc), h) <= 1e-12, s
            pre = c["x"][:, s, None].double() * cell.weight_ih.t() + cell.bias_ih + cell.bias_hh + h_prev @ cell.weight_hh.t()
            want = torch.cat([torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])], 1)
            assert _rel(ref["gates"][:, s], want) <= 1e-12, s
        assert _rel(ref["h_last"], h) <= 1e-12


def test_lstm_ref_float32_is_a_float32_evaluation():
    """The yardstick run stays in float32 end to end and sits where fp32 rounding puts it: not equal to float64, within 1e-5 of it."""
    c, ref, y32 = TR.lstm_case_refs(3, 17, 33, 7)
    for k in TR.LSTM_OUTPUTS:
        assert y32[k].dtype == torch.float32 and ref[k].dtype == F64
        e = TR.yardstick(ref[k], y32[k])
        assert 0.0 < e < 1e-5, (k, e)


def test_lstm_dw_hh_of_steps_sums_to_dw_hh():
    """the per-step terms of dw_hh over all samples and steps are dw_hh; the first step's term is 0 (h_0 = 0)"""
    B, T, H = 3, 9, 5
    c, ref, _ = TR.lstm_case_refs(B, T, H, 59)
    args = (c["x"], c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"], c["dh_last"])
    total = sum(TR.lstm_dw_hh_of_steps(*args, b, 0, 4) + TR.lstm_dw_hh_of_steps(*args, b, 4, T) for b in range(B))
    assert _rel(total, ref["dw_hh"]) <= 1e-12
    assert float(TR.lstm_dw_hh_of_steps(*args, 1, 0, 1).abs().max()) == 0.0


def test_lstm_ref_reproduces_the_recorded_828_step_encoder():
    """g11_temporal_828.npz (nn.LSTM of the original project, fp32, T = 828, H = 96): embedding and every gradient at the tolerances
    tests/test_oracle_golden.py holds the oracle to on this fixture (1e-5 / 1e-4)."""
    d = load_npz("g11_temporal_828.npz")
    sd, grads = sub(d, "sd"), sub(d, "grad")
    x, demb = t(d["ts"]), t(d["demb"]).double()
    p = [sd[f"lstm.{k}"].double().requires_grad_(True) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    _, _, h = TR.lstm_ref(x, *p, F64)
    lin = TR.linear_ref(h.detach(), sd["fc.weight"], sd["fc.bias"], demb)
    assert rel_err(lin["out"], t(d["emb"])) < 1e-5
    g = torch.autograd.grad(h, p, lin["dx"])
    for k, v in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), g):
        assert rel_err(v, grads[f"lstm.{k}"]) < 1e-4, k
    assert rel_err(lin["dw"], grads["fc.weight"]) < 1e-4 and rel_err(lin["db"], grads["fc.bias"]) < 1e-4


@pytest.mark.parametrize("N,F,D", [(1, 1, 1), (3, 96, 64), (50, 7, 1)])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_ref_equals_torch(N, F, D, bias):
    g = torch.Generator().manual_seed(N + F + D)
    x = torch.randn((N, F), generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn((D, F), generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn((D,), generator=g, dtype=F64).requires_grad_(True) if bias else None
    dout = torch.randn((N, D), generator=g, dtype=F64)
    ref = TR.linear_ref(x.detach(), w.detach(), None if b is None else b.detach(), dout)
    out = torch.nn.functional.linear(x, w, b)
    out.backward(dout)
    assert _rel(ref["out"], out.detach()) <= 1e-12 and _rel(ref["dx"], x.grad) <= 1e-12 and _rel(ref["dw"], w.grad) <= 1e-12
    if bias:
        assert _rel(ref["db"], b.grad) <= 1e-12


@pytest.mark.parametrize("N,F,Hd,D", [(1, 4, 32, 8), (50, 4, 32, 64), (7, 4, 5, 3)])
def test_meta_mlp_ref_equals_torch(N, F, Hd, D):
    """Against Linear -> ReLU -> Linear in double, with one pre-activation of exactly 0 (integer data): its dhidden is 0, as torch's."""
    g = torch.Generator().manual_seed(N + F + Hd + D)
    net = torch.nn.Sequential(torch.nn.Linear(F, Hd), torch.nn.ReLU(), torch.nn.Linear(Hd, D)).double()
    md = torch.randint(-4, 5, (N, F), generator=g).double()
    with torch.no_grad():
        net[0].weight.copy_(torch.randint(-4, 5, (Hd, F), generator=g).double())
        net[0].bias.copy_(torch.randint(-4, 5, (Hd,), generator=g).double())
        net[0].weight[1 % Hd] = 0
        net[0].weight[1 % Hd, 0] = 1
        md[0, 0] = -net[0].bias[1 % Hd]
    demb = torch.randn((N, D), generator=g, dtype=F64)
    ref = TR.meta_mlp_ref(md, net[0].weight.detach(), net[0].bias.detach(), net[2].weight.detach(), net[2].bias.detach(), demb)
    assert float(ref["pre"][0, 1 % Hd]) == 0.0 and float(ref["dhidden"][0, 1 % Hd]) == 0.0
    hid = net[1](net[0](md))
    hid.retain_grad()
    emb = net[2](hid)
    emb.backward(demb)
    assert _rel(ref["hidden"], hid.detach()) <= 1e-12 and _rel(ref["emb"], emb.detach()) <= 1e-12
    for k, p in (("dw0", net[0].weight), ("db0", net[0].bias), ("dw2", net[2].weight), ("db2", net[2].bias)):
        assert _rel(ref[k], p.grad) <= 1e-12, k
    assert _rel(ref["dhidden"], hid.grad * (hid.detach() > 0)) <= 1e-12


def test_yardstick_normalisation():
    a = torch.tensor([1.0, -4.0, 2.0], dtype=F64)
    assert TR.yardstick(a, a.float()) == 0.0
    assert TR.yardstick(a, torch.tensor([1.0, -4.0, 3.0])) == 0.25
    assert TR.yardstick(torch.zeros(3, dtype=F64), torch.zeros(3)) == 0.0
    assert TR.yardstick(torch.zeros(3, dtype=F64), torch.tensor([0.0, 1e-9, 0.0])) == float("inf")
