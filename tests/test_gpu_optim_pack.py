"""The fused optimizer step (csrc/optim.hip: ``opt_pack_kernel`` behind ``mau_opt_pack_step`` / ``mau_adamw_pack_step``) and the weight
packs (csrc/conv3x3.hip: ``pack_tile`` behind ``mau_conv3x3_pack_weights`` / ``_multi``) through the C ABI, against the float64 rules and
the placement of tests/optim_pack_ref.py (checked on the CPU by tests/test_optim_pack_host.py).

Ten layer shapes, the smallest at which a 64 x 64 x 9 block kernel with 16-channel chunks can go wrong (``optim_pack_ref.SHAPES``), always
all of them in ONE table, rows varying over (wf, wd), (wf, NULL), (NULL, wd) and (NULL, NULL).  Every buffer a launch touches is a slot
of a larger allocation (``Arena``) that holds a NaN of fixed payload, in the buffer's own type, in front of, between and behind the
slots and in the pack slots themselves: what a launch must write is decided by ``pack_ref``'s mask, what it must leave alone still has
the sentinel's bits afterwards, and the gradients -- the kernel's const input -- have theirs.

SGD on the dyadic inputs, the moments of Adam / AdamW on theirs, and every pack are held to the reference BIT FOR BIT; the Adam-family
parameter, and the moments on random data, to the rule ``optim_pack_ref.adam_bound`` (K = 16 roundings, counted there), which prints the
worst err / bound before it asserts.

Measured on one MI355X, worst err / bound (K = 16) over every case of this module, with the case (t, shape) it occurred in; none needs
more than K = 6.1:
    rule    w, dyadic inputs      w, production          w, grad_scale = 1/3   exp_avg          exp_avg_sq       (with grad_scale)
    Adam    0.126 (12, 64x64)     0.337 (100000, 130x72)  0.091 (10, 130x72)    0.114 (1, 64x65)  0.163 (1, 17x200)  0.140 / 0.248
    AdamW   0.110 (12, 72x130)    0.380 (100000, 130x72)  0.134 (10, 72x130)    0.114 (1, 64x65)  0.163 (1, 17x200)  0.140 / 0.248
The largest figures are at t = 100000, where both amplification terms have vanished and the bound is the bare count of roundings.
"""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

from tests import optim_pack_ref as R
from tests._helpers import _call, _stream, bits, mau, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 64                  # sentinel elements in front of and between the slots (a multiple of 16 bytes in every type: the packs are
                            # written in 16-byte vectors)
TAIL = 1 << 16              # sentinel elements behind the last slot: more than one 16-channel chunk of the widest pack (9 x 256 x 16)
SENTINEL = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FD5, torch.float16: 0x7E55}       # quiet NaNs with a payload
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
F32 = torch.float32
MODES = [(True, True), (True, False), (False, True), (False, False)]                        # (wf, wd) of a table row


def _code(dt):
    from mau_amd import _lib
    return {torch.float32: _lib.MAU_F32, torch.bfloat16: _lib.MAU_BF16, torch.float16: _lib.MAU_F16}[dt]


class Arena:
    """slots of ``sizes`` elements of ``dt`` in one allocation, the sentinel everywhere else -- and in the slots until ``set``"""

    def __init__(self, sizes, dt):
        self.dt, self.sizes, self.off = dt, list(sizes), []
        o = GUARD
        for n in self.sizes:
            self.off.append(o)
            o += -(-n // GUARD) * GUARD + GUARD
        self.host = torch.full((o + TAIL,), SENTINEL[dt], dtype=_INT[dt]).view(dt)
        self.inside = torch.zeros(o + TAIL, dtype=torch.bool)
        for o, n in zip(self.off, self.sizes):
            self.inside[o:o + n] = True
        self.dev = None

    def set(self, i, x):
        self.host[self.off[i]:self.off[i] + self.sizes[i]] = x.reshape(-1).to(self.dt)
        return self

    def cuda(self):
        self.dev = self.host.cuda()
        return self

    def ptr(self, i):
        if self.dev is None:
            self.cuda()
        return self.dev.data_ptr() + self.off[i] * self.dev.element_size()

    def back(self):
        """the whole allocation after the launches; nothing outside the slots may have been written"""
        torch.cuda.synchronize()
        r = self.dev.cpu()
        assert bool((bits(r)[~self.inside] == SENTINEL[self.dt]).all()), "elements outside the buffer were written"
        return r

    def slot(self, r, i):
        return r[self.off[i]:self.off[i] + self.sizes[i]]


def _untouched(x, dt):
    return bool((bits(x) == SENTINEL[dt]).all())


def _scalar(value):
    """a device float between two sentinels -> (tensor, address of the float)"""
    t = torch.full((3,), SENTINEL[F32], dtype=torch.int32).view(F32)
    t[1] = value
    t = t.cuda()
    return t, t.data_ptr() + 4


def _device_table(host):
    return torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).cuda()


@functools.lru_cache(maxsize=None)
def _exact(shape):
    return R.exact_case(*shape)


@functools.lru_cache(maxsize=None)
def _random(shape):
    return R.random_case(*shape)


def _tiles_opt(shape):
    return (R.pad64(shape[0]) // 64) * (R.pad64(shape[1]) // 64)


# ---- the packs alone ----------------------------------------------------------------------------------------------------------------------
def _pack_sizes(shapes):
    return [R.packed_elems(co, ci) for co, ci in shapes], [R.packed_elems(ci, co) for co, ci in shapes]


def _assert_pack(got, w, dt, which, passed, what):
    """a pack slot after a launch: ``pack_ref`` of ``w`` where the mask says written, the sentinel elsewhere; all sentinel if not passed"""
    if not passed:
        assert _untouched(got, dt), what + (which, "a buffer that was not passed was written")
        return
    want, mask = R.pack_ref(w, dt, which)
    want = torch.where(mask, bits(want), torch.tensor(SENTINEL[dt], dtype=_INT[dt])).view(dt)
    assert same_bits(got, want), what + (which,)


def _pack_single(w_arena, i, shape, dt, mode, wf=None, wd=None, j=0):
    """mau_conv3x3_pack_weights of slot i of ``w_arena`` into slot j of (new, or the given) pack arenas; a buffer is passed per ``mode``"""
    nf, nd = _pack_sizes([shape])
    wf, wd = wf or Arena(nf, dt).cuda(), wd or Arena(nd, dt).cuda()
    _call("mau_conv3x3_pack_weights", w_arena.ptr(i), wf.ptr(j) if mode[0] else None, wd.ptr(j) if mode[1] else None, _code(dt), shape[0], shape[1],
          _stream())
    return wf, wd


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_pack_weights_layout(mau, shape, dt):
    """mau_conv3x3_pack_weights with wf only, wd only and both, on random weights and on the dyadic ties of round-to-nearest-even: the
    bits of ``pack_ref`` (zero pads included), nothing outside the buffer, a buffer that was not passed left alone, w unchanged"""
    from mau_amd._lib import lib
    assert lib.mau_conv3x3_kc(_code(dt)) == R.KC
    assert lib.mau_conv3x3_packed_elems(_code(dt), shape[0], shape[1]) == R.packed_elems(shape[0], shape[1])
    assert lib.mau_conv3x3_packed_elems(_code(dt), shape[1], shape[0]) == R.packed_elems(shape[1], shape[0])
    for kind, w in (("random", R.random_weights(*shape)), ("ties", R.tie_weights(*shape))):
        wa = Arena([w.numel()], F32).set(0, w).cuda()
        for mode in MODES[:3]:
            wf, wd = _pack_single(wa, 0, shape, dt, mode)
            for which, arena, passed in (("wf", wf, mode[0]), ("wd", wd, mode[1])):
                _assert_pack(arena.slot(arena.back(), 0), w, dt, which, passed, (shape, kind, mode))
        assert same_bits(wa.back(), wa.host), (shape, kind, "w was written")


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
def test_pack_weights_table(mau, dt):
    """all ten shapes in one mau_conv3x3_pack_desc_fill table, rows alternating (wf, wd), (wf, NULL), (NULL, wd) -- every shape in every
    form over the three rotations --, one mau_conv3x3_pack_weights_multi: the bits of the single-launch form and of ``pack_ref``;
    the table's tile count is the sum of the rows' tiles"""
    from mau_amd._lib import lib
    ws = [R.tie_weights(*s, seed=1) if i % 2 else R.random_weights(*s, seed=1) for i, s in enumerate(R.SHAPES)]
    wa = Arena([w.numel() for w in ws], F32)
    for i, w in enumerate(ws):
        wa.set(i, w)
    wa.cuda()
    nf, nd = _pack_sizes(R.SHAPES)
    for rot in range(3):
        modes = [MODES[(i + rot) % 3] for i in range(len(ws))]
        wf, wd, wf1, wd1 = (Arena(n, dt).cuda() for n in (nf, nd, nf, nd))
        host = ctypes.create_string_buffer(lib.mau_conv3x3_pack_desc_bytes() * len(ws))
        nxt, tiles = ctypes.c_int(0), 0
        for i, (s, m) in enumerate(zip(R.SHAPES, modes)):
            _call("mau_conv3x3_pack_desc_fill", ctypes.addressof(host), i, wa.ptr(i), wf.ptr(i) if m[0] else None, wd.ptr(i) if m[1] else None, _code(dt),
                  s[0], s[1], nxt.value, ctypes.addressof(nxt))
            tiles += m[0] * (R.pad64(s[0]) // 64) * -(-s[1] // R.KC) + m[1] * (R.pad64(s[1]) // 64) * -(-s[0] // R.KC)
            assert nxt.value == tiles, (i, s, m)
            _pack_single(wa, i, s, dt, m, wf1, wd1, i)
        table = _device_table(host)
        _call("mau_conv3x3_pack_weights_multi", table.data_ptr(), len(ws), nxt.value, _code(dt), _stream())
        got_f, got_d = wf.back(), wd.back()
        assert same_bits(got_f, wf1.back()) and same_bits(got_d, wd1.back()), (rot, "table form against single launches")
        for i, (s, m) in enumerate(zip(R.SHAPES, modes)):
            _assert_pack(wf.slot(got_f, i), ws[i], dt, "wf", m[0], (s, rot))
            _assert_pack(wd.slot(got_d, i), ws[i], dt, "wd", m[1], (s, rot))
    assert same_bits(wa.back(), wa.host), "w was written"


# ---- the optimizer step -----------------------------------------------------------------------------------------------------------------------
class Step:
    """One table of ``shapes`` for mau_opt_pack_step: w, g (and m, v where ``moments`` names them) from ``cases``, the packs of ``dt``
    per ``modes`` (a pack that is not in the row keeps its slot, which must stay untouched)."""

    def __init__(self, shapes, cases, dt, modes, moments):
        from mau_amd._lib import lib
        self.shapes, self.dt, self.modes, self.moments = list(shapes), dt, list(modes), moments
        n = [co * ci * 9 for co, ci in self.shapes]
        self.a = {k: Arena(n, F32) for k in ("w", "g") + tuple(moments)}
        for k, key in (("w", "p"), ("g", "g"), ("m", "m"), ("v", "v")):
            if k in self.a:
                for i, c in enumerate(cases):
                    self.a[k].set(i, R.to_f32(c[key]))
                self.a[k].cuda()
        nf, nd = _pack_sizes(self.shapes)
        self.a["wf"], self.a["wd"] = Arena(nf, dt).cuda(), Arena(nd, dt).cuda()
        host = ctypes.create_string_buffer(lib.mau_adamw_pack_desc_bytes() * len(self.shapes))
        nxt, tiles = ctypes.c_int(0), 0
        for i, (s, md) in enumerate(zip(self.shapes, self.modes)):
            _call("mau_opt_pack_desc_fill", ctypes.addressof(host), i, self.a["w"].ptr(i), self.a["g"].ptr(i), self.a["m"].ptr(i) if "m" in self.a else None,
                  self.a["v"].ptr(i) if "v" in self.a else None, self.a["wf"].ptr(i) if md[0] else None, self.a["wd"].ptr(i) if md[1] else None, s[0], s[1],
                  nxt.value, ctypes.addressof(nxt))
            tiles += _tiles_opt(s)
            assert nxt.value == tiles, (i, s)
        self.tiles, self.table = tiles, _device_table(host)
        self.keep = []

    def launch(self, rule, *, step=None, grad_scale=None, lr, beta1, beta2=0.0, eps=0.0, wd=0.0, nesterov=False, adamw_entry=False):
        st = _scalar(float(step)) if step is not None else (None, None)
        gs = _scalar(grad_scale) if grad_scale is not None else (None, None)
        self.keep += [st[0], gs[0]]
        if adamw_entry:
            assert rule == R.ADAMW and grad_scale is None
            _call("mau_adamw_pack_step", self.table.data_ptr(), len(self.shapes), self.tiles, _code(self.dt), st[1], lr, beta1, beta2, eps, wd, _stream())
        else:
            _call("mau_opt_pack_step", self.table.data_ptr(), len(self.shapes), self.tiles, _code(self.dt), rule, st[1], gs[1], lr, beta1, beta2, eps, wd,
                  int(nesterov), _stream())
        return self

    def read(self):
        """{name: the whole arena}, sentinels checked, and g with the bits it came with"""
        raw = {k: a.back() for k, a in self.a.items()}
        assert same_bits(raw["g"], self.a["g"].host), "the gradients were written"
        for t in self.keep:
            assert t is None or (_untouched(t.cpu()[[0, 2]], F32)), "a device scalar's neighbours were written"
        return raw

    def layer(self, raw, k, i):
        x = self.a[k].slot(raw[k], i)
        return x.reshape(*self.shapes[i], 3, 3) if k in ("w", "g", "m", "v") else x

    def check_packs(self, raw, what):
        """wf / wd of every row: ``pack_ref`` of the kernel's own new w, and the bits mau_conv3x3_pack_weights makes of that w in
        equally pre-filled buffers; the slot of a pack that is not in the row untouched"""
        nf, nd = _pack_sizes(self.shapes)
        wf1, wd1 = Arena(nf, self.dt).cuda(), Arena(nd, self.dt).cuda()
        for i, (s, md) in enumerate(zip(self.shapes, self.modes)):
            w = self.layer(raw, "w", i)
            _assert_pack(self.layer(raw, "wf", i), w, self.dt, "wf", md[0], what + (s, md))
            _assert_pack(self.layer(raw, "wd", i), w, self.dt, "wd", md[1], what + (s, md))
            if md[0] or md[1]:
                _pack_single(self.a["w"], i, s, self.dt, md, wf1, wd1, i)
        assert same_bits(raw["wf"], wf1.back()) and same_bits(raw["wd"], wd1.back()), what + ("against mau_conv3x3_pack_weights",)


def _modes(rot, n=len(R.SHAPES)):
    return [MODES[(i + rot) % 4] for i in range(n)]


def _same_raw(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), what + (k,)


# ---- SGD, exact -------------------------------------------------------------------------------------------------------------------------------
def _sgd_hyper(cfg):
    return dict(lr=R.SGD_EXACT["lr"], beta1=R.SGD_EXACT["beta1"] if cfg["momentum"] else 0.0, wd=cfg["wd"], nesterov=cfg["nesterov"])


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "grad_scale"])
@pytest.mark.parametrize("config", list(R.SGD_CONFIGS))
def test_sgd_exact(mau, config, scaled, dt):
    """two consecutive launches on the dyadic inputs: w and the momentum buffer equal ``step_ref`` rounded to float32 bit for bit after
    each (plain: the rows' m is NULL), the packs follow the new w, a row without packs is updated all the same"""
    cfg = R.SGD_CONFIGS[config]
    rot = list(R.SGD_CONFIGS).index(config) * 2 + scaled + R.DTYPES.index(dt)
    cases = [_exact(s) for s in R.SHAPES]
    hyper = _sgd_hyper(cfg)
    gs = R.SGD_EXACT_SCALE if scaled else None
    S = Step(R.SHAPES, cases, dt, _modes(rot), "m" if cfg["momentum"] else "")
    ref = [(c["p"], c["m"] if cfg["momentum"] else None) for c in cases]
    for launch in (1, 2):
        raw = S.launch(R.SGD, grad_scale=gs, **hyper).read()
        for i, (s, c) in enumerate(zip(R.SHAPES, cases)):
            p, m, _ = R.step_ref(R.SGD, ref[i][0], c["g"], ref[i][1], None, grad_scale=gs, **hyper)
            ref[i] = (p, m)
            assert same_bits(S.layer(raw, "w", i), R.to_f32(p)), (config, scaled, launch, s, "w")
            if m is not None:
                assert same_bits(S.layer(raw, "m", i), R.to_f32(m)), (config, scaled, launch, s, "momentum buffer")
        S.check_packs(raw, (config, scaled, launch))


@pytest.mark.parametrize("config", list(R.SGD_CONFIGS))
def test_sgd_grad_scale_is_a_factor_of_g(mau, config):
    """grad_scale -> 1.0 gives the bits of grad_scale = NULL, grad_scale -> 1/2 those of a launch on a halved g; g itself is not rewritten"""
    cfg, dt = R.SGD_CONFIGS[config], torch.bfloat16
    cases = [_exact(s) for s in R.SHAPES]
    halved = [dict(c, g=c["g"] * 0.5) for c in cases]
    hyper, moments = _sgd_hyper(cfg), "m" if cfg["momentum"] else ""
    res = {}
    for name, cs, gs in (("null", cases, None), ("one", cases, 1.0), ("half", cases, 0.5), ("halved g", halved, None)):
        S = Step(R.SHAPES, cs, dt, _modes(1), moments)
        res[name] = S.launch(R.SGD, grad_scale=gs, **hyper).launch(R.SGD, grad_scale=gs, **hyper).read()
        res[name].pop("g")
    _same_raw(res["one"], res["null"], (config, "grad_scale -> 1"))
    _same_raw(res["half"], res["halved g"], (config, "grad_scale -> 1/2"))
    assert not same_bits(res["half"]["w"], res["null"]["w"])


# ---- Adam / AdamW --------------------------------------------------------------------------------------------------------------------------------
_worst = {}


def _within(got, ref, bound, key, what):
    """|got - ref| <= bound in every element; prints the worst err / bound before it asserts"""
    err = np.abs(got.double().numpy() - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f"RATIO {key:24s} {what}: worst err / bound {ratio:.4f} (K = {R.K:g}: {ratio * R.K:.2f} roundings; so far {_worst[key]:.4f})")
    assert ratio <= 1.0, (key, what, ratio)
    return ratio


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("wd", [0.0, R.ADAM_EXACT_WD], ids=["wd0", "wd0.25"])
@pytest.mark.parametrize("rule", ["adam", "adamw"])
def test_adam_exact_moments(mau, rule, wd, dt):
    """the dyadic Adam inputs at t = 1, 2, 7, 12, the device step scalar filled directly: exp_avg and exp_avg_sq equal the reference
    bit for bit, the parameter lies within the rule, the packs follow the new
    w; mau_adamw_pack_step gives the bits of mau_opt_pack_step(MAU_OPT_ADAMW, grad_scale = NULL)"""
    code = R.RULES[rule]
    cases = [_exact(s) for s in R.SHAPES]
    for rot, t in enumerate(R.EXACT_STEPS):
        S = Step(R.SHAPES, cases, dt, _modes(rot + R.DTYPES.index(dt)), "mv")
        raw = S.launch(code, step=t, wd=wd, **R.ADAM_EXACT).read()
        for i, (s, c) in enumerate(zip(R.SHAPES, cases)):
            tr = {}
            p, m, v = R.step_ref(code, c["p"], c["g"], c["m"], c["v"], step=t, wd=wd, trace=tr, **R.ADAM_EXACT)
            assert same_bits(S.layer(raw, "m", i), R.to_f32(m)), (rule, wd, t, s, "exp_avg")
            assert same_bits(S.layer(raw, "v", i), R.to_f32(v)), (rule, wd, t, s, "exp_avg_sq")
            _within(S.layer(raw, "w", i), p, R.adam_bound(p, tr), f"{rule} exact w", (wd, t, s))
        S.check_packs(raw, (rule, wd, t))
        if rule == "adamw":
            S2 = Step(R.SHAPES, cases, dt, S.modes, "mv")
            _same_raw(S2.launch(code, step=t, wd=wd, adamw_entry=True, **R.ADAM_EXACT).read(), raw, ("mau_adamw_pack_step", wd, t))


def _production_hyper(mau, rule):
    sig = inspect.signature({"adam": mau.Adam, "adamw": mau.AdamW}[rule].__init__).parameters
    h = dict(lr=sig["lr"].default, beta1=sig["betas"].default[0], beta2=sig["betas"].default[1], eps=sig["eps"].default, wd=sig["weight_decay"].default)
    assert (h["beta1"], h["beta2"]) == (0.9, 0.999) and h["eps"] > 0 and h["wd"] == {"adam": 0.0, "adamw": 1e-2}[rule]
    return h


def _production(mau, rule, dt, t, gs, rot):
    code, hyper = R.RULES[rule], _production_hyper(mau, rule)
    cases = [_random(s) for s in R.SHAPES]
    S = Step(R.SHAPES, cases, dt, _modes(rot), "mv")
    raw = S.launch(code, step=t, grad_scale=gs, **hyper).read()
    tag = "" if gs is None else " grad_scale"
    for i, (s, c) in enumerate(zip(R.SHAPES, cases)):
        tr = {}
        p, m, v = R.step_ref(code, c["p"], c["g"], c["m"], c["v"], step=t, grad_scale=gs, trace=tr, **hyper)
        bm, bv = R.moment_bounds(tr)
        _within(S.layer(raw, "m", i), m, bm, f"{rule}{tag} exp_avg", (t, s))
        _within(S.layer(raw, "v", i), v, bv, f"{rule}{tag} exp_avg_sq", (t, s))
        _within(S.layer(raw, "w", i), p, R.adam_bound(p, tr), f"{rule}{tag} w", (t, s))
        zero = (c["g"] == 0) & (c["v"] == 0)                  # the update is m / eps there
        assert zero.any() or c["g"].size < 256
        assert bool((S.layer(raw, "v", i).numpy()[zero] == 0).all())
    S.check_packs(raw, (rule, t, gs))


@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("rule", ["adam", "adamw"])
def test_adam_production_hyper_parameters(mau, rule, dt):
    """the defaults of mau_amd.Adam / AdamW (betas 0.9 / 0.999) on random p, g, m and v >= 0 over several decades, v = 0 with g = 0
    among them (the update is m / eps), t = 1 .. 100000 (1 - 0.999^1 cancels three digits; 0.9^100000 is 0): w, exp_avg and
    exp_avg_sq within the rule, the packs the bits of the new w -- infinities of fp16 included"""
    for rot, t in enumerate(R.PRODUCTION_STEPS):
        _production(mau, rule, dt, t, None, rot + R.DTYPES.index(dt))


@pytest.mark.parametrize("rule", ["adam", "adamw"])
def test_adam_inexact_grad_scale(mau, rule):
    """grad_scale -> 1/3: one more rounding in g, inside the count of the rule"""
    _production(mau, rule, torch.bfloat16, 10, 1.0 / 3.0, 2)


# ---- block ownership ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.DTYPES, ids=R.DT_IDS)
@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_block_ownership(mau, rule, dt):
    """(130, 72) as the second row of a table (tile0 = 2 behind a (65, 64) layer, and 6 behind a (130, 72) one without packs) and alone:
    the same bits in w, the state and both packs of that layer -- a row's blocks are numbered from its own tile0"""
    shape = (130, 72)
    if rule == "sgd":
        kw, moments, case = dict(grad_scale=0.5, lr=R.SGD_EXACT["lr"], beta1=0.5, wd=0.25, nesterov=True), "m", _exact
    else:
        kw, moments, case = dict(step=7, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2), "mv", _random
    code = R.RULES[rule]
    one = Step([shape], [case(shape)], dt, [MODES[0]], moments)
    raw1 = one.launch(code, **kw).read()
    one.check_packs(raw1, (rule, "alone"))
    for first, mode in (((65, 64), MODES[0]), (shape, MODES[3])):
        two = Step([first, shape], [case(first), case(shape)], dt, [mode, MODES[0]], moments)
        raw2 = two.launch(code, **kw).read()
        for k in raw1:
            assert same_bits(two.layer(raw2, k, 1), one.layer(raw1, k, 0)), (rule, first, k)
        two.check_packs(raw2, (rule, first))
