"""CPU-only checks of tests/optim_pack_ref.py, the references tests/test_gpu_optim_pack.py holds the fused optimizer step
(csrc/optim.hip) and the weight packs (csrc/conv3x3.hip) against: ``step_ref`` against torch.optim.SGD / Adam / AdamW in float64 (an
oracle that is wrong proves nothing on the GPU), ``pack_ref`` as a placement that inverts, and the proof that every intermediate of the
dyadic cases is a float32 -- which is what lets the GPU test demand bits.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from tests import optim_pack_ref as R

F64 = np.float64


# ---- step_ref against torch, float64 ------------------------------------------------------------------------------------------------------
TORCH_CASES = {
    "sgd": (R.SGD, torch.optim.SGD, dict(lr=0.05)),
    "sgd_momentum": (R.SGD, torch.optim.SGD, dict(lr=0.05, momentum=0.9)),
    "sgd_nesterov": (R.SGD, torch.optim.SGD, dict(lr=0.05, momentum=0.9, nesterov=True)),
    "sgd_wd": (R.SGD, torch.optim.SGD, dict(lr=0.05, weight_decay=0.01)),
    "sgd_nesterov_wd": (R.SGD, torch.optim.SGD, dict(lr=0.05, momentum=0.7, nesterov=True, weight_decay=0.01)),
    "adam": (R.ADAM, torch.optim.Adam, dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8)),
    "adam_wd": (R.ADAM, torch.optim.Adam, dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)),
    "adamw": (R.ADAMW, torch.optim.AdamW, dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0)),
    "adamw_wd": (R.ADAMW, torch.optim.AdamW, dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)),
}


def _rel(got, want):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("name", list(TORCH_CASES))
def test_step_ref_against_torch_float64(name):
    """three consecutive steps with a new gradient each: parameter and state equal torch's single-tensor implementation to 1e-12
    relative; the hyper-parameters are the same unrounded Python floats on both sides"""
    rule, cls, kw = TORCH_CASES[name]
    r = np.random.default_rng(11)
    shape = (5, 7, 3, 3)
    p0 = r.standard_normal(shape)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = cls([tp], foreach=False, **kw)
    momentum = kw.get("momentum", 0.0)
    hyper = dict(lr=kw["lr"], wd=kw.get("weight_decay", 0.0), f32_hyper=False)
    if rule == R.SGD:
        hyper.update(beta1=momentum, nesterov=kw.get("nesterov", False))
        m, v = (np.zeros(shape) if momentum else None), None       # a zero buffer: the first step gives buf = g, torch's rule
    else:
        hyper.update(beta1=kw["betas"][0], beta2=kw["betas"][1], eps=kw["eps"])
        m, v = np.zeros(shape), np.zeros(shape)
    p = p0
    for t in (1, 2, 3):
        g = r.standard_normal(shape) * 0.3
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.step_ref(rule, p, g, m, v, step=t, **hyper)
        assert _rel(p, tp.detach().numpy()) <= 1e-12, (name, t, "p")
        st = opt.state[tp]
        if rule == R.SGD:
            if momentum:
                assert _rel(m, st["momentum_buffer"].numpy()) <= 1e-12, (name, t, "momentum_buffer")
        else:
            assert float(st["step"]) == t
            assert _rel(m, st["exp_avg"].numpy()) <= 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12, (name, t, "moments")


def test_step_ref_grad_scale_and_hyper_rounding():
    """grad_scale is a factor of g in front of everything; the hyper-parameters enter as float32 values"""
    c = R.random_case(3, 5)
    kw = dict(step=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
    a = R.step_ref(R.ADAMW, c["p"], c["g"], c["m"], c["v"], grad_scale=1.0 / 3.0, **kw)
    b = R.step_ref(R.ADAMW, c["p"], c["g"] * R.f32(1.0 / 3.0), c["m"], c["v"], **kw)
    assert all((x == y).all() for x, y in zip(a, b))
    rounded = {k: (R.f32(x) if k != "step" else x) for k, x in kw.items()}
    assert rounded["lr"] != kw["lr"]
    b = R.step_ref(R.ADAMW, c["p"], c["g"], c["m"], c["v"], f32_hyper=False, **rounded)
    a = R.step_ref(R.ADAMW, c["p"], c["g"], c["m"], c["v"], **kw)
    assert all((x == y).all() for x, y in zip(a, b))


# ---- pack_ref is a placement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_pack_ref_is_a_placement(shape, dt):
    """every (co, ci, tap) once in each pack, everything else zero, the inverse of the placement returns w (values exact in the type)"""
    Cout, Cin = shape
    w = R.exact_values(Cout, Cin, dt)
    assert bool((w != 0).all()) and torch.equal(w.to(dt).float(), w)
    for which, rows, k in (("wf", Cout, Cin), ("wd", Cin, Cout)):
        pack, mask = R.pack_ref(w, dt, which)
        assert pack.dtype == dt and pack.numel() == R.packed_elems(rows, k) == mask.numel() and bool(mask.all())
        idx = R.pack_index(Cout, Cin, dt, which)
        held = idx[idx >= 0]
        assert held.numel() == w.numel() and torch.equal(held.sort().values, torch.arange(w.numel()))
        assert bool((pack[idx < 0] == 0).all()) and int((pack != 0).sum()) == w.numel()
        back = torch.zeros(w.numel())
        back[held] = pack[idx >= 0].float()
        assert torch.equal(back.reshape(w.shape), w), (shape, which)
        # the chunk, the tap and the 16-lane slot of every weight, from the header's sentence; the row is the permutation's business
        pos = torch.arange(idx.numel())[idx >= 0]
        co, ci, tap = held // (Cin * 9), held // 9 % Cin, held % 9
        kk, row, tp = (ci, co, tap) if which == "wf" else (co, ci, 8 - tap)
        rp = R.pad64(rows)
        assert torch.equal(pos % 16, kk % 16) and torch.equal(pos // (16 * rp * 9), kk // 16) and torch.equal(pos // (16 * rp) % 9, tp)
        q = pos // 16 % rp
        assert torch.equal(q // 64, row // 64)
        want = q % 64 if dt == torch.float32 else 2 * (q % 32) + q % 64 // 32
        assert torch.equal(row % 64, want), (shape, which, "row permutation")


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", [(3, 5), (16, 23), (65, 17)], ids=["3x5", "16x23", "65x17"])
def test_pack_ref_against_the_element_loop(shape, dt):
    """the vectorised placement against the loop that writes one element at a time, values rounded to the type (random, and ties)"""
    for w in (R.random_weights(*shape), R.tie_weights(*shape)):
        for which in ("wf", "wd"):
            got, want = R.pack_ref(w, dt, which)[0], R.pack_loop(w, dt, which)
            assert got.dtype == want.dtype and torch.equal(got.float(), want.float()), (shape, which)


def test_tie_weights_are_ties():
    """a good share of the dyadic weights lies exactly between two neighbours of bf16 / fp16, with both parities of the kept bit, so
    that rounding up, down, or away from zero each disagree with round-to-nearest-even somewhere"""
    w = R.tie_weights(64, 64).double().reshape(-1)
    for dt, bits in ((torch.bfloat16, 8), (torch.float16, 11)):
        e = torch.floor(torch.log2(w.abs()))
        units = w.abs() / 2.0 ** (e - bits)                   # in halves of a unit of the type's last place: odd = an exact tie
        tie = (units == units.round()) & (units.long() % 2 == 1)
        assert float(tie.double().mean()) > 0.25, (dt, float(tie.double().mean()))
        r = w.float().to(dt).double()[tie]
        up = r.abs() > w.abs()[tie]
        assert 0.25 < float(up.double().mean()) < 0.75, dt     # nearest-even goes both ways
        last = (r.abs() / 2.0 ** (e[tie] - bits + 1)).round().long() % 2
        assert bool((last == 0).all()) or bool((r.abs() == 2.0 ** (e[tie] + 1)).logical_or(last == 0).all()), dt


# ---- the dyadic cases are exact in float32 -------------------------------------------------------------------------------------------------
def _assert_all_f32(trace, what):
    for name, x in trace.items():
        assert R.is_f32(x), what + (name,)


def test_exact_inputs_lie_on_their_grids():
    c = R.exact_case(72, 130)
    for name, unit, lo, hi in (("p", 8, -16, 16), ("g", 4, -8, 8), ("m", 8, -16, 16), ("v", 16, 0, 32)):
        k = c[name] * unit
        assert (k == np.round(k)).all() and k.min() == lo and k.max() == hi, name
    assert not np.signbit(c["p"]).any() or (c["p"][np.signbit(c["p"])] != 0).all()      # no negative zero among the inputs


@pytest.mark.parametrize("config", list(R.SGD_CONFIGS))
@pytest.mark.parametrize("scaled", [False, True], ids=["", "grad_scale"])
def test_sgd_exact_case_is_exact(config, scaled):
    """two consecutive steps: every product, sum and result survives float32 unchanged, so a fused or an unfused multiply-add, in any
    order of the kernel's choice, gives these very bits"""
    cfg = R.SGD_CONFIGS[config]
    for shape in ((17, 200), (72, 130)):
        c = R.exact_case(*shape)
        p, m = c["p"], (c["m"] if cfg["momentum"] else None)
        for launch in (1, 2):
            tr = {}
            p, m, _ = R.step_ref(R.SGD, p, c["g"], m, None, lr=R.SGD_EXACT["lr"], beta1=R.SGD_EXACT["beta1"] if cfg["momentum"] else 0.0,
                                 wd=cfg["wd"], nesterov=cfg["nesterov"], grad_scale=R.SGD_EXACT_SCALE if scaled else None, trace=tr)
            assert ("buf" in tr) == cfg["momentum"] and ("g_nesterov" in tr) == cfg["nesterov"] and ("g_scaled" in tr) == scaled
            _assert_all_f32(tr, (config, scaled, shape, launch))
            assert np.abs(p).max() < 4.0 + 2.0 * launch


@pytest.mark.parametrize("rule", ["adam", "adamw"])
@pytest.mark.parametrize("wd", [0.0, R.ADAM_EXACT_WD])
def test_adam_exact_case_is_exact(rule, wd):
    """m, v, the decayed p (or the gradient with its L2 term), every product in front of them and both bias corrections are float32s
    for t = 1, 2, 7, 12 (4^t - 3^t < 2^24); the update itself is not, which is why the parameter has a tolerance and the moments none"""
    for shape in ((17, 200), (72, 130)):
        c = R.exact_case(*shape)
        for t in R.EXACT_STEPS:
            tr = {}
            R.step_ref(R.RULES[rule], c["p"], c["g"], c["m"], c["v"], step=t, wd=wd, trace=tr, **R.ADAM_EXACT)
            rest = {k: x for k, x in tr.items() if k not in ("update", "p")}
            assert {"m", "v", "bc1", "bc2", "b1_t", "b2_t"} <= set(rest) and ("p_decayed" in rest) == (rule == "adamw")
            assert ("g_decayed" in rest) == (rule == "adam" and wd != 0.0)
            _assert_all_f32(rest, (rule, wd, shape, t))
            assert (tr["v"] >= 0).all() and tr["bc2"] == (4.0 ** t - 3.0 ** t) / 4.0 ** t and tr["bc1"] == 1.0 - 2.0 ** -t
    assert 4 ** 12 - 3 ** 12 < 2 ** 24 <= 4 ** 13 - 3 ** 13


def test_tolerance_rule_figures():
    """the amplification terms of the rule at the production betas: 9 + 499.5 at t = 1, nothing left at t = 100000"""
    c = R.random_case(3, 5)
    for t, want in ((1, 1.0 + 9.0 + 0.5 * 999.0), (100000, 1.0)):
        tr = {}
        p, _, _ = R.step_ref(R.ADAMW, c["p"], c["g"], c["m"], c["v"], step=t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, trace=tr)
        amp = (R.adam_bound(p, tr) / (R.K * R.E32) - np.abs(p)) / np.abs(tr["update"])
        assert np.allclose(amp, want, rtol=1e-4), (t, float(amp.max()))      # (0.999 as a float32 is 0.99899995)
        bm, bv = R.moment_bounds(tr)
        same = np.sign(tr["b1_m"]) * np.sign(tr["omb1_g"]) >= 0
        assert np.allclose(bm[same], R.K * R.E32 * np.abs(tr["m"])[same], rtol=1e-12) and (bm >= R.K * R.E32 * np.abs(tr["m"]) * (1 - 1e-12)).all()
        assert (bv == R.K * R.E32 * tr["v"]).all()
    assert R.K <= 16
