"""Native gradient clipping on a real MI355X: lmv_grad_norm against a float64 norm, the coefficient and the skip of non-finite steps, lmv_adamw_flat_clip
against torch.optim.AdamW fed the scaled / clamped gradient, and FlatAdamW(clip_grad=...) on a whole model against torch.nn.utils.clip_grad_norm_ in front of
an unclipped step -- what the reference's training loops call (engine.py:82-95)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor

DEV = "cuda:0"


def ops():
    from lemevit_amd import ops as _ops
    return _ops


def new_stat():
    return torch.zeros(ops().GRAD_STAT_FLOATS, device=DEV)


def norm64(segs):
    return float(torch.linalg.vector_norm(torch.cat([s.reshape(-1).double() for s in segs])))


def rel(a, b):
    return abs(a - b) / abs(b)


@functools.lru_cache(maxsize=None)
def table_case():
    """Segment 0 of 2 CH + 4 elements (16-byte aligned) and 129 small segments of 1, 3, 10, 257, ... elements: views at ODD element offsets of one buffer,
    so 4-byte aligned only -- 130 segments, more than one by-value table (96 segments, csrc/misc.hip).  Returns (segments, buffer of the small ones, float64 norm);
    shared by the tests below, never written."""
    CH = ops().NORM_CHUNK
    big = det_tensor((2 * CH + 4,), "clip.big", 3, 0.02).to(DEV)
    lens = [(1, 3, 10, 257)[i % 4] for i in range(129)]
    buf = det_tensor((sum(lens) + 3 * len(lens) + 8,), "clip.small", 3).to(DEV)
    segs, off = [big], 1
    for n in lens:
        segs.append(buf[off:off + n])
        off += n
        off += 1 - (off & 1) + 2 * (n & 1)          # the next start is odd again, and the gaps vary
    assert off <= buf.numel() and [s.numel() for s in segs[1:]] == lens
    assert all((s.data_ptr() & 7) == 4 for s in segs[1:]) and big.data_ptr() % 16 == 0
    return segs, buf, norm64(segs)


def single_lengths():
    CH = 16384          # = ops().NORM_CHUNK (asserted in the test: a parametrisation cannot load the library at collection time)
    return [4, CH - 4, CH, CH + 4, 3 * CH + 8]


# ---- 1. the norm against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", single_lengths())
def test_grad_norm_single_segment(n):
    """|norm - norm64| <= 1e-5 norm64: a tree sum of non-negative fp32 terms is off by at most (depth + 2) 2^-24 relative, depth <= 30 gives ~2e-6 before the
    square root -- a 5x margin.  A second call is bit-identical in all of stat."""
    o = ops()
    assert o.NORM_CHUNK == 16384
    g = det_tensor((n,), "clip.single", n, 0.05).to(DEV)
    st = o.grad_norm([g], 0.0, new_stat())
    ref = norm64([g])
    print(f"n={n}: norm {float(st[0]):.9g} vs float64 {ref:.9g} (rel {rel(float(st[0]), ref):.2e})")
    assert rel(float(st[0]), ref) <= 1e-5
    st2 = o.grad_norm([g], 0.0, new_stat())
    assert torch.equal(st, st2)
    assert st.tolist()[1:] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_grad_norm_segment_table():
    o = ops()
    segs, _, ref = table_case()
    st = o.grad_norm(segs, 0.0, new_stat())
    print(f"table: norm {float(st[0]):.9g} vs float64 {ref:.9g} (rel {rel(float(st[0]), ref):.2e})")
    assert rel(float(st[0]), ref) <= 1e-5
    assert torch.equal(st, o.grad_norm(segs, 0.0, new_stat()))
    # the partition depends on the lengths alone: the same values at 16-byte aligned addresses give the same bits
    moved = [segs[0].clone()] + [s.clone() for s in segs[1:]]
    assert all(s.data_ptr() % 16 == 0 for s in moved)
    assert torch.equal(st, o.grad_norm(moved, 0.0, new_stat()))


# ---- 2. the coefficient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2.0, 0.5, 0.0, -1.0])
def test_grad_norm_coefficient(factor):
    o = ops()
    segs, _, ref = table_case()
    max_norm = factor * ref
    st = o.grad_norm(segs, max_norm, new_stat()).tolist()
    want = min(1.0, max_norm / (ref + 1e-6)) if max_norm > 0 else 1.0
    print(f"max_norm {max_norm:.6g}: coef {st[1]:.9g} vs {want:.9g}; coef * (1 / coef) - 1 = {st[1] * st[2] - 1:.2e}")
    assert rel(st[1], want) <= 1e-5
    assert abs(st[2] * st[1] - 1.0) <= 1e-6
    assert (st[1] == 1.0) == (factor != 0.5) and st[3] == 0.0 and st[4] == 0.0


# ---- 3. non-finite values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_grad_norm_non_finite(bad):
    o = ops()
    segs, _, ref = table_case()
    last = segs[-1].clone()
    last[-1] = bad
    segs = list(segs[:-1]) + [last]
    step = torch.full((), 5, device=DEV, dtype=torch.int32)
    st = new_stat()
    o.grad_norm(segs, 0.5 * ref, st, skip_nonfinite=True, step_dev=step)
    assert st.tolist()[1:5] == [0.0, float("inf"), 1.0, 1.0] and not torch.isfinite(st[0]) and int(step) == 5
    o.grad_norm(segs, 0.5 * ref, st, skip_nonfinite=True, step_dev=step)
    assert float(st[3]) == 1.0 and float(st[1]) == 0.0 and float(st[4]) == 2.0 and int(step) == 5
    # a skipped step leaves the flat update's buffers alone
    n = 4096 * 3
    p = det_tensor((n,), "p", 7).to(DEV); g = det_tensor((n,), "g", 7, 0.1).to(DEV)
    m = det_tensor((n,), "m", 7, 0.01).to(DEV); v = det_tensor((n,), "v", 7, 0.01).abs().to(DEV)
    shadow = p.to(torch.bfloat16)
    before = [t.clone() for t in (p, m, v, shadow)]
    o.adamw_flat(p, g, m, v, None, 1e-2, 0.9, 0.999, 1e-8, 0.05, 0, shadow=shadow, step_dev=step, stat=st)
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v, shadow)))
    # a clean table under the same flag: the step count moves, nothing is skipped
    clean = o.grad_norm(table_case()[0], 0.5 * ref, new_stat(), skip_nonfinite=True, step_dev=step)
    assert int(step) == 6 and clean.tolist()[3:5] == [0.0, 0.0] and rel(float(clean[1]), 0.5) <= 1e-5
    # without the flag the norm flows through as in torch
    st2 = o.grad_norm(segs, 0.5 * ref, new_stat(), step_dev=step)
    assert float(st2[3]) == 1.0 and not torch.isfinite(st2[0]) and float(st2[4]) == 0.0 and int(step) == 7
    want = torch.clamp(torch.tensor(0.5 * ref, dtype=torch.float32) / (st2[0].cpu() + 1e-6), max=1.0)       # 0 for inf, NaN for NaN
    assert torch.equal(torch.nan_to_num(st2[1].cpu(), nan=-7.0), torch.nan_to_num(want, nan=-7.0))


# ---- 4. the flat update with a coefficient / a clamp ---------------------------------------------------------------------------------------
def _adamw_err(transform, **kw):
    """max-abs difference, relative to max |p|, between three lmv_adamw_flat(_clip) steps (keywords kw) and torch.optim.AdamW fed transform(g)"""
    o = ops()
    n = 4096 * 3
    p = det_tensor((n,), "p", 7).to(DEV); g = det_tensor((n,), "g", 7, 0.1).to(DEV)
    pr = torch.nn.Parameter(p.clone()); opt = torch.optim.AdamW([pr], lr=1e-2, betas=(0.9, 0.999), eps=1e-2, weight_decay=0.05)
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    shadow = torch.zeros(n, device=DEV, dtype=torch.bfloat16)
    for step in range(1, 4):
        pr.grad = transform(g.clone()); opt.step()
        o.adamw_flat(p, g, m, v, None, 1e-2, 0.9, 0.999, 1e-2, 0.05, step, shadow=shadow, **kw)
    assert torch.isfinite(p).all() and torch.equal(shadow, p.to(torch.bfloat16))
    return float((p - pr.detach()).abs().max()) / float(pr.detach().abs().max())


def test_adamw_flat_with_coefficient_and_clamp():
    """eps = 1e-2 makes the update depend on the gradient's magnitude (at 1e-8 Adam's step is nearly scale-invariant and a dropped coefficient would not
    show); tolerance 1e-5 of max |p|, test_adamw_flat's own; the control -- the same reference against an unscaled / unclamped update -- must miss it."""
    coef = torch.tensor(0.37, dtype=torch.float32)
    st = new_stat()
    st[1], st[2] = coef, 1.0 / coef
    one = new_stat()
    one[1], one[2] = 1.0, 1.0
    e = _adamw_err(lambda g: g * coef.to(DEV), stat=st)
    c = _adamw_err(lambda g: g * coef.to(DEV), stat=one)
    print(f"adamw_flat stat coef 0.37: rel err {e:.3e} (control with coef 1: {c:.3e})")
    assert e <= 1e-5 < c
    e = _adamw_err(lambda g: g.clamp(-0.05, 0.05), clip_value=0.05)
    c = _adamw_err(lambda g: g.clamp(-0.05, 0.05))
    print(f"adamw_flat clip_value 0.05: rel err {e:.3e} (control without: {c:.3e})")
    assert e <= 1e-5 < c
    assert _adamw_err(lambda g: g, stat=one) == _adamw_err(lambda g: g)          # a coefficient of 1 is the plain update


# ---- 5 - 9. whole model ----------------------------------------------------------------------------------------------------------------------
def _twin(**kw):
    import lemevit_amd
    torch.manual_seed(0)
    m = lemevit_amd.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
    return m, lemevit_amd.FlatAdamW(m, lr=1e-3, eps=1e-3, weight_decay=0.05, **kw)


@functools.lru_cache(maxsize=None)
def _batch():
    return det_tensor((4, 3, 64, 64), "clip.img", 1).to(DEV), torch.tensor([3, 8, 1, 6], device=DEV)


def _backward(m, opt):
    x, y = _batch()
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", torch.bfloat16):
        loss = torch.nn.functional.cross_entropy(m(x), y)
    loss.backward()


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _flat_names(opt):
    return {n for n, _, _, _ in opt._slices}


CASES = ["half", "small"]


@functools.lru_cache(maxsize=None)
def model_case(kind="half"):
    """Computed once per kind, read by tests 5, 6 and 8.  "half": c = half the gradient norm of step 1, the prescribed case (clipping is active there; the later
    norms fall below c, coefficient 1).  "small": c = 1.0, below the norm of every step (asserted by the tests), so every one of the three steps clips.  Holds
    the parameters, norms and coefficients of twin A (FlatAdamW(clip_grad=c)) after 3 steps, of a second run of A, of twin B (plain FlatAdamW,
    torch.nn.utils.clip_grad_norm_ in front of step()) and of the unclipped twin C."""
    if kind == "half":
        m, opt = _twin()
        _backward(m, opt)
        c = 0.5 * float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for p in m.parameters()])))
    else:
        c = 1.0
    out = {"c": c}
    for name, kw in (("A", dict(clip_grad=c)), ("A2", dict(clip_grad=c)), ("B", {}), ("C", {})):
        m, opt = _twin(**kw)
        norms, coefs = [], []
        for _ in range(3):
            _backward(m, opt)
            if name == "B":
                norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), c)))
            opt.step()
            if name != "B":
                norms.append(float(opt.grad_norm))
                coefs.append(float(opt._stat[1]))
        out[name] = (_params(m), norms, _flat_names(opt))
        out[name + ".coef"] = coefs
    return out


@pytest.mark.parametrize("kind", CASES)
def test_flat_adamw_clip_matches_torch_clip_grad_norm(kind):
    """Twin A against twin B.  The gradients of the two are bit-identical and only the coefficient's rounding differs: the norms agree to 1e-5 relative on
    every step, every parameter to 1e-6 max(1, |p|max) (three steps of at most a few lr each, times 1e-5: ~1e-7).  Control: the unclipped twin C is further
    than that from A on a block parameter and on a non-block parameter.  Two runs of A agree bit for bit.  "half" is the prescribed threshold (one clipped
    step, then two with coefficient 1: norms 16.56, 2.08, 2.47 against c = 8.28), "small" clips on every step."""
    case = model_case(kind)
    (pa, na, flat), (pa2, na2, _), (pb, nb, _), (pc, ncl, _) = case["A"], case["A2"], case["B"], case["C"]
    print(f"{kind}: clip_grad {case['c']:.6g}; norms native {na} torch {nb} unclipped twin {ncl}; native coefficients {case['A.coef']}")
    assert all(v == 0.0 for v in ncl), "an optimizer without options must not compute the norm"
    if kind == "half":
        assert rel(nb[0], 2.0 * case["c"]) <= 1e-5, "c is half the norm of step 1: clipping is active there (later norms may fall below c: coefficient 1)"
        assert case["A.coef"][0] < 1.0
    else:
        assert all(n > case["c"] for n in nb) and all(k < 1.0 for k in case["A.coef"]), "clipping must be active on every step"
    for a, b in zip(na, nb):
        assert rel(a, b) <= 1e-5, (na, nb)
    worst = max((float((pa[n] - pb[n]).abs().max()) / max(1.0, float(pb[n].abs().max())), n) for n in pa)
    print(f"A vs B: worst parameter difference {worst[0]:.3e} of max(1, |p|max) at {worst[1]}")
    for n in pa:
        d = float((pa[n] - pb[n]).abs().max())
        assert d <= 1e-6 * max(1.0, float(pb[n].abs().max())), f"{n}: {d:.3e}"
    far = {n for n in pa if float((pa[n] - pc[n]).abs().max()) > 1e-6 * max(1.0, float(pc[n].abs().max()))}
    assert far & flat and far - flat, "control: the unclipped twin must differ on block and non-block parameters"
    assert na == na2 and all(torch.equal(pa[n], pa2[n]) for n in pa)


@pytest.mark.parametrize("kind", CASES)
def test_clip_grad_norm_call_then_step(kind):
    """opt.clip_grad_norm_(c); opt.step() on a plain FlatAdamW equals constructor-side clipping bit for bit; the gradients in memory are not rescaled;
    zero_grad() disarms the coefficient."""
    case = model_case(kind)
    m, opt = _twin()
    for i in range(3):
        _backward(m, opt)
        g0 = opt._flat_g.clone()
        norm = opt.clip_grad_norm_(case["c"])
        assert norm.dim() == 0 and float(norm) == case["A"][1][i] and opt._armed
        assert float(opt._stat[1]) == case["A.coef"][i]
        assert torch.equal(g0, opt._flat_g)
        opt.step()
        assert not opt._armed
    pa = case["A"][0]
    got = _params(m)
    assert all(torch.equal(pa[n], got[n]) for n in pa)
    assert opt.state_dict()["step"] == 3
    with pytest.raises(ValueError):
        opt.clip_grad_norm_(1.0, norm_type=1.0)
    _backward(m, opt)
    opt.clip_grad_norm_(case["c"])
    opt.zero_grad()
    assert not opt._armed


def test_skipped_step_leaves_everything_unchanged():
    m, opt = _twin(skip_nonfinite=True)
    _backward(m, opt)
    opt.step()
    assert int(opt.skipped_steps) == 0 and float(opt.grad_norm) > 0 and opt.state_dict()["step"] == 1
    _backward(m, opt)
    flat = _flat_names(opt)
    named = dict(m.named_parameters())
    blk = named[sorted(flat)[0]]
    other = named[sorted(n for n in named if n not in flat and named[n].grad is not None)[0]]
    blk.grad.view(-1)[1] = float("inf")
    other.grad.view(-1)[0] = float("inf")

    def snapshot():
        rest = opt._rest.state_dict()["state"]
        return ([p.detach().clone() for p in m.parameters()] + [opt._exp_avg.clone(), opt._exp_avg_sq.clone(), opt._shadow.clone()] +
                [wt.clone() for _, wt in opt._tpairs] +
                [v.clone() for k in sorted(rest) for kk, v in sorted(rest[k].items()) if torch.is_tensor(v)])
    before, named_before, step_before = snapshot(), _params(m), opt.state_dict()["step"]
    opt.step()
    after = snapshot()
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
    assert opt.state_dict()["step"] == step_before == 1
    assert int(opt.skipped_steps) == 1 and not torch.isfinite(opt.grad_norm)
    _backward(m, opt)
    opt.step()
    assert int(opt.skipped_steps) == 1 and opt.state_dict()["step"] == 2 and torch.isfinite(opt.grad_norm)
    moved = {n for n, p in m.named_parameters() if not torch.equal(p.detach(), named_before[n])}
    assert moved & flat and moved - flat, "the next clean step must move block and non-block weights"
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_clipped_step_under_graph_capture():
    """One eager step (the warm-up of the capture) and two replays of the captured clipped step leave the parameters of three eager steps with the same
    clip_grad from the same state, bit for bit.  clip_grad is the "small" one, below the norm of every step: the capture pass launches nothing, so the two
    replays are steps 2 and 3, and both must clip -- the coefficient read after the last replay is < 1 and is the eager twin's, which a replay that ignored the
    device coefficient, or one frozen at capture time, would miss."""
    from lemevit_amd.graph import GraphedStep
    case = model_case("small")
    m, opt = _twin(clip_grad=case["c"])
    g = GraphedStep(lambda: (_backward(m, opt), opt.step()), warmup=1)
    g()
    torch.cuda.synchronize()
    assert float(opt.grad_norm) == case["A"][1][1] and float(opt._stat[1]) == case["A.coef"][1] < 1.0
    g()
    torch.cuda.synchronize()
    ops().check_stage_errors("graph replay", sync=False)
    pa, na, _ = case["A"]
    coefs = case["A.coef"]
    assert all(k < 1.0 for k in coefs[1:]) and coefs[1] != coefs[2], "both replayed steps clip, each with a coefficient of its own"
    got = _params(m)
    assert all(torch.equal(pa[n], got[n]) for n in pa)
    norm = float(opt.grad_norm)
    assert norm > 0 and norm == na[2] and float(opt._stat[1]) == coefs[2] and opt.state_dict()["step"] == 3
    pc = case["C"][0]
    assert any(not torch.equal(pc[n], got[n]) for n in got), "control: the unclipped twin ends elsewhere"


def test_clip_value_mode():
    """clip_mode='value' clamps inside the flat update and with a multi-tensor clamp on the other gradients -- against torch.nn.utils.clip_grad_value_ in front
    of a plain step; no reduction launch."""
    c = 1e-3
    m1, o1 = _twin(clip_grad=c, clip_mode="value")
    m2, o2 = _twin()
    for _ in range(2):
        _backward(m1, o1)
        o1.step()
        _backward(m2, o2)
        assert max(float(p.grad.abs().max()) for p in m2.parameters()) > c, "the clamp must be active"
        torch.nn.utils.clip_grad_value_(m2.parameters(), c)
        o2.step()
    assert float(o1.grad_norm) == 0.0
    p1, p2 = _params(m1), _params(m2)
    for n in p1:
        d = float((p1[n] - p2[n]).abs().max())
        assert d <= 1e-6 * max(1.0, float(p2[n].abs().max())), f"{n}: {d:.3e}"


def test_default_path_untouched(monkeypatch):
    """With no option set step() calls neither new entry point, and is bit-identical to a second plain optimizer on a twin."""
    o = ops()

    def boom(*a, **k):
        raise AssertionError("the unclipped step must not reach the clipping entry points")
    m1, o1 = _twin()
    m2, o2 = _twin()
    _backward(m2, o2)
    o2.step()
    monkeypatch.setattr(o, "grad_norm", boom)
    monkeypatch.setattr(o.lib, "lmv_adamw_flat_clip", boom)
    monkeypatch.setattr(o.lib, "lmv_grad_norm", boom)
    _backward(m1, o1)
    o1.step()
    p1, p2 = _params(m1), _params(m2)
    assert all(torch.equal(p1[n], p2[n]) for n in p1)
    assert float(o1.grad_norm) == 0.0 and o1.state_dict()["step"] == 1
