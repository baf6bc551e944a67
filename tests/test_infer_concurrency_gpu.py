"""The concurrency INSIDE one no-grad eval forward (lemevit_amd/model.py: forward_features / _stages_from / _tail_split), on a real MI355X.

Two schedules are on by default in every inference pass:
* the TAIL SPLIT (model._INFER_TAIL_PARTS): from the second pass at an input shape, for B >= 32, the stages behind the last persistent stage kernel and the classifier tail run as
  sub-batches on forked streams and are joined with torch.cat -- decided by LeMeViT._whole_seen (written by the previous pass), ordered by a fork event, the `cold` flag and
  record_stream;
* the SIDE STREAM (model._INFER_SIDE): the meta-token MLP of stage i > 0 on blocks.aux_streams(dev, 1)[0] next to the transition convolution.

The yardstick of every bit-equality below is the SINGLE-STREAM REFERENCE: the same pass with blocks.aux_streams patched to hand out the current stream -- the same kernels on the same
sub-batches, one after the other.  A race, a missing join or a mis-ordered cat shows as a difference from it; against the whole-batch pass 1 only the bf16 end-to-end budget (5e-2 of
the logits' max-abs, as in test_model_gpu.py) can hold, because other row counts select other GEMM kernels.  Every test that claims to cross the split counts the calls of
LeMeViT._tail_split and fails on zero."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict
from oracle import lemevit_oracle as O

DEV = "cuda:0"
BF16_E2E = 5e-2          # test_model_forward_bf16 / test_split_forward_concurrent_sub_batches


def close(out, ref, tol, what):
    out = np.asarray(out.detach().float().cpu().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), what
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max()
    assert err <= tol * mx, f"{what}: max-abs err {err:.3e} > {tol:.0e} * {mx:.3e}"
    return err / mx


_models, _images, _oracle_rows = {}, {}, {}


def _model(variant):
    """One instance per variant for the whole file (filling LeMeViT-Base's state_dict takes seconds), handed out as a model that has not seen any input shape yet."""
    import lemevit_amd
    m = _models.get(variant)
    if m is None:
        m = lemevit_amd.create_model(variant, num_classes=1000)
        m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 3))
        m = _models[variant] = m.to(DEV).eval()
    torch.cuda.synchronize()
    m.__dict__.pop("_whole_seen", None)
    return m


def _image(res, B):
    """The first B of one fixed set of images per resolution (so that B = 32 and B = 33 share rows, and the oracle is computed once)."""
    n = 64 if res == 224 else 32
    assert B <= n
    img = _images.get(res)
    if img is None:
        img = _images[res] = det_tensor((n, 3, res, res), f"inferconc.img{res}", 4).to(DEV)
    return img[:B]


def _oracle_logits(m, rows):
    """float64 oracle logits of LeMeViT-Tiny (m: the instance under test, for its weights) on the given rows of the 224 x 224 images: computed once per row."""
    todo = [r for r in rows if r not in _oracle_rows]
    if todo:
        sd = {k: (v.detach().double().cpu() if v.dtype.is_floating_point else v.detach().cpu()) for k, v in m.state_dict().items()}
        with torch.no_grad():
            y = O.lemevit_forward(sd, O.VARIANTS["lemevit_tiny"], _image(224, 64)[todo].double().cpu())
        assert y.dtype == torch.float64
        for r, v in zip(todo, y):
            _oracle_rows[r] = v
    return torch.stack([_oracle_rows[r] for r in rows])


def _fwd(m, img, bf16=True):
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16, enabled=bf16):
        return m(img)


def _reference(monkeypatch, m, img, bf16=True):
    """The single-stream reference: every auxiliary stream is the current one."""
    import lemevit_amd.blocks as BL
    with monkeypatch.context() as mp:
        mp.setattr(BL, "aux_streams", lambda dev, n: [torch.cuda.current_stream(dev)] * n)
        y = _fwd(m, img, bf16)
    torch.cuda.synchronize()
    return y


class _SplitSpy:
    """Counts LeMeViT._tail_split: per call the stage it starts at, the rows of its sub-batches, launches.concurrent at entry and whether a hipGraph capture was under way."""

    def __init__(self, monkeypatch):
        import lemevit_amd.model as M
        self.calls, self.inside = [], 0
        orig, spy = M.LeMeViT._tail_split, self

        def tail_split(model, i, xt, H, W, c, st):
            parts = max(1, min(st["tail_parts"], xt.shape[0]))
            spy.calls.append({"stage": i, "rows": [t.shape[0] for t in xt.chunk(parts)], "concurrent": M.launches.concurrent,
                              "capturing": torch.cuda.is_current_stream_capturing()})
            spy.inside += 1
            try:
                return orig(model, i, xt, H, W, c, st)
            finally:
                spy.inside -= 1

        monkeypatch.setattr(M.LeMeViT, "_tail_split", tail_split)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


class _AuxSpy:
    """Counts blocks.aux_streams (the only source of forked streams of the inference pass) and calls through."""

    def __init__(self, monkeypatch):
        import lemevit_amd.blocks as BL
        self.calls = []
        orig = BL.aux_streams

        def aux_streams(dev, n):
            self.calls.append(n)
            return orig(dev, n)

        monkeypatch.setattr(BL, "aux_streams", aux_streams)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


_busy_mat = []


def _busy():
    """A few 4096 x 4096 fp32 matmuls on the current stream: it lags, and a forked stream that does not wait for it runs ahead of whatever it still has to write."""
    if not _busy_mat:
        _busy_mat.append(det_tensor((4096, 4096), "inferconc.busy", 1).to(DEV))
    a = _busy_mat[0]
    with torch.autocast("cuda", enabled=False):
        for _ in range(4):
            a = (a @ a) * 1e-2
    return a


def _seen(m):
    """(key, tuple) of the ONE input shape the model has recorded."""
    (key, seen), = m.__dict__.get("_whole_seen", {}).items()
    return key, seen


def _rows(B, parts):
    return [t.shape[0] for t in torch.empty(B).chunk(parts)]


# ---- 1. the tail split against the single-stream run (bit for bit), the whole-batch pass (bf16 budget) and the float64 oracle -------------------------------------------------------
@pytest.mark.parametrize("variant,res,B", [("lemevit_tiny", 224, 32), ("lemevit_tiny", 224, 33), ("lemevit_base", 224, 32), ("lemevit_base", 224, 33), ("lemevit_tiny", 384, 32)])
def test_tail_split_bit_equal_to_single_stream(monkeypatch, variant, res, B):
    """Pass 1 at a shape runs whole and records the persistent stages (Tiny 224: "S" in front of the tail; Base 224: "D" and "S"; Tiny 384: "S2"); passes 2 and 3 split stage 4 and the
    classifier tail into two sub-batches (B = 33: 17 + 16 rows, which may pick different GEMM kernels per half).  Passes 2 and 3 are bit-equal to each other and to the single-stream
    reference, and inside the bf16 end-to-end budget of pass 1.  Tiny 224: the first and last image of each sub-batch against the float64 oracle, at the same budget -- a mis-joined or
    mis-ordered cat would move exactly those rows, and the oracle does not share code with the split."""
    m, img, spy = _model(variant), _image(res, B), _SplitSpy(monkeypatch)
    p1 = _fwd(m, img)
    assert spy.take() == [], "pass 1 at a new shape must run whole"
    key, seen = _seen(m)
    assert key[0] == (3, res, res) and len(seen) == m.num_stages and seen[3] and not seen[4], (key, seen)
    p2 = _fwd(m, img)
    p3 = _fwd(m, img)
    torch.cuda.synchronize()
    calls = spy.take()
    assert [c["stage"] for c in calls] == [4, 4] and all(c["rows"] == _rows(B, 2) for c in calls), calls          # once per pass, behind the last persistent stage
    ref = _reference(monkeypatch, m, img)
    assert [c["rows"] for c in spy.take()] == [_rows(B, 2)], "the reference runs the same sub-batches"
    assert _seen(m) == (key, seen)
    assert p2.shape == p1.shape == (B, 1000)
    assert torch.equal(p2, p3), float((p2.float() - p3.float()).abs().max())
    assert torch.equal(p2, ref), float((p2.float() - ref.float()).abs().max())
    assert torch.equal(p3, ref)
    e2 = close(p2, p1, BF16_E2E, "pass 2 (split) vs pass 1 (whole)")
    close(p3, p1, BF16_E2E, "pass 3 (split) vs pass 1 (whole)")
    print(f"{variant} {res} B={B}: split pass 2 vs whole pass 1 rel err {e2:.2e}")
    if variant == "lemevit_tiny" and res == 224:
        cuts = np.cumsum([0] + _rows(B, 2))
        edge = sorted({int(r) for a, b in zip(cuts[:-1], cuts[1:]) for r in (a, b - 1)})          # B = 32: rows 0, 15, 16, 31
        want = _oracle_logits(m, edge)
        eo = close(p2[edge], want, BF16_E2E, f"split logits, rows {edge}, vs float64 oracle")
        e1 = close(p1[edge], want, BF16_E2E, f"whole-batch logits, rows {edge}, vs float64 oracle")
        print(f"{variant} {res} B={B}: rows {edge} vs float64 oracle: split rel err {eo:.2e}, whole rel err {e1:.2e}")


# ---- 2. more than two parts ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_tail_split_four_parts(monkeypatch):
    """_INFER_TAIL_PARTS = 4: three auxiliary streams, 8 rows each."""
    import lemevit_amd.model as M
    monkeypatch.setattr(M, "_INFER_TAIL_PARTS", 4)
    m, img, spy, aux = _model("lemevit_tiny"), _image(224, 32), _SplitSpy(monkeypatch), _AuxSpy(monkeypatch)
    p1 = _fwd(m, img)
    assert spy.take() == []
    aux.take()
    p2 = _fwd(m, img)
    torch.cuda.synchronize()
    assert [c["rows"] for c in spy.take()] == [[8, 8, 8, 8]]
    assert 3 in aux.take(), "the split must have asked for three auxiliary streams"
    ref = _reference(monkeypatch, m, img)
    assert [c["rows"] for c in spy.take()] == [[8, 8, 8, 8]]
    assert torch.equal(p2, ref), float((p2.float() - ref.float()).abs().max())
    close(p2, p1, BF16_E2E, "four sub-batches vs whole batch")


# ---- 3. _whole_seen is keyed without B -------------------------------------------------------------------------------------------------------------------------------------------------
def test_first_pass_at_new_batch_size_splits(monkeypatch):
    """The record of an input shape does not carry B: a pass at B = 4 (cannot split) teaches the model the shape, and the FIRST pass at B = 32 splits at once -- with per-stream
    scratch (model._persistent, ops._workspace) that has never been used at that size: both caches start empty here, as in a fresh process."""
    import lemevit_amd.model as M
    from lemevit_amd import ops
    m, spy = _model("lemevit_tiny"), _SplitSpy(monkeypatch)
    torch.cuda.synchronize()          # nothing in flight reads the scratch that is dropped here
    M._scratch_cache.clear(); ops._ws_cache.clear()
    _fwd(m, _image(224, 4))
    assert spy.take() == []
    key, seen = _seen(m)
    assert key[0] == (3, 224, 224) and seen[3] and not seen[4]
    img = _image(224, 32)
    first = _fwd(m, img)
    torch.cuda.synchronize()
    assert [c["rows"] for c in spy.take()] == [[16, 16]], "the first pass at B = 32 of a known shape must split"
    ref = _reference(monkeypatch, m, img)
    assert len(spy.take()) == 1
    assert torch.equal(first, ref), float((first.float() - ref.float()).abs().max())


# ---- 4. cold operand caches under a busy chip ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lemevit_tiny", "lemevit_base"])
def test_tail_split_cold_caches_busy_chip(monkeypatch, variant):
    """test_split_forward_cold_caches for the inner split: after new_training_pass() every derived operand (bf16 casts, LayerNorm and conv + BatchNorm folds, the packed stages, the
    classifier tail) is rebuilt by the next pass -- those of the tail by sub-batch 0, on a current stream that lags behind four large matmuls.  The other sub-batch streams must wait for
    them (`cold`), and the casts of the meta-token MLPs, built on the side stream, must be joined.  Three cold passes (allocator reuse of the per-stream blocks included), each bit-equal
    to the WARM single-stream reference."""
    import lemevit_amd.model as M
    m, img, spy = _model(variant), _image(224, 32), _SplitSpy(monkeypatch)
    _fwd(m, img)
    ref = _reference(monkeypatch, m, img)
    assert len(spy.take()) == 1
    for rep in range(3):
        fills = M.cache_fills()
        M.new_training_pass()
        _busy()
        cold = _fwd(m, img)
        torch.cuda.synchronize()
        assert M.cache_fills() > fills, "the pass rebuilt no operand: it was not cold"
        assert [c["rows"] for c in spy.take()] == [[16, 16]]
        assert torch.equal(cold, ref), (rep, float((cold.float() - ref.float()).abs().max()))


# ---- 5. side stream on versus off ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,bf16", [("lemevit_tiny", True), ("lemevit_base", True), ("lemevit_tiny", False)])
def test_side_stream_on_equals_off(monkeypatch, variant, bf16):
    """B = 4 cannot split, so only the side path differs: the meta-token MLP of stages 1 .. 4 on the auxiliary stream next to the transition convolution, or in line.  The same kernels
    on the same operands: logits bit-equal, warm and on the first pass after new_training_pass() under a busy chip (the MLP's casts are then BUILT on the side stream)."""
    import lemevit_amd.model as M
    m, img, spy, aux = _model(variant), _image(224, 4), _SplitSpy(monkeypatch), _AuxSpy(monkeypatch)
    monkeypatch.setattr(M, "_INFER_SIDE", False)
    off = _fwd(m, img, bf16)
    torch.cuda.synchronize()
    assert aux.take() == [], "side path off: no stream may be forked at B = 4"
    monkeypatch.setattr(M, "_INFER_SIDE", True)
    on = _fwd(m, img, bf16)
    torch.cuda.synchronize()
    forks = aux.take()
    assert forks and set(forks) == {1}, forks          # the side path ran (one fork per stage transition), and nothing else forked
    assert torch.equal(on, off), float((on.float() - off.float()).abs().max())
    fills = M.cache_fills()
    M.new_training_pass()
    _busy()
    cold_on = _fwd(m, img, bf16)
    torch.cuda.synchronize()
    assert M.cache_fills() > fills and len(aux.take()) == len(forks)
    assert torch.equal(cold_on, off), float((cold_on.float() - off.float()).abs().max())
    monkeypatch.setattr(M, "_INFER_SIDE", False)
    M.new_training_pass()
    _busy()
    cold_off = _fwd(m, img, bf16)
    torch.cuda.synchronize()
    assert aux.take() == [] and torch.equal(cold_off, off)
    assert spy.take() == []


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_tail_split_under_graph_capture(monkeypatch):
    """GraphedStep(warmup=2) around an eval forward: warm-up pass 1 runs whole, warm-up pass 2 and the CAPTURED pass split -- the forks become branches of the hipGraph.  Three replays,
    each bit-equal to the eager single-stream reference."""
    from lemevit_amd import ops
    from lemevit_amd.graph import GraphedStep
    m, img, spy = _model("lemevit_tiny"), _image(224, 32), _SplitSpy(monkeypatch)
    outs = []

    def step():
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            outs[:] = [m(img)]

    g = GraphedStep(step, warmup=2)
    calls = spy.take()
    assert [(c["rows"], c["capturing"]) for c in calls] == [([16, 16], False), ([16, 16], True)], calls
    got = []
    for _ in range(3):
        g()
        ops.check_stage_errors("test_tail_split_under_graph_capture", sync=True)
        got.append(outs[0].clone())
    torch.cuda.synchronize()
    assert spy.take() == []          # replays issue nothing from Python
    ref = _reference(monkeypatch, m, img)
    assert len(spy.take()) == 1
    for r, y in enumerate(got):
        assert torch.equal(y, ref), (r, float((y.float() - ref.float()).abs().max()))


# ---- 7. negative controls --------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,bf16", [(224, False), (96, True)])
def test_no_split_without_a_persistent_stage(monkeypatch, res, bf16):
    """fp32 (the stage kernels are bf16) and 96 x 96 bf16 (no stage kernel takes that shape): nothing runs as a persistent launch, so there is no last one to split behind -- not in
    pass 1 and not in pass 2, although B = 32."""
    m, spy = _model("lemevit_tiny"), _SplitSpy(monkeypatch)
    img = _image(224, 32) if res == 224 else det_tensor((32, 3, 96, 96), "inferconc.img96", 4).to(DEV)
    a = _fwd(m, img, bf16)
    b = _fwd(m, img, bf16)
    torch.cuda.synchronize()
    assert spy.take() == []
    key, seen = _seen(m)
    assert key[0] == (3, res, res) and not any(seen), (key, seen)
    assert torch.equal(a, b)


def test_no_inner_concurrency_inside_split_forward(monkeypatch):
    """graph.split_forward already fills the streams a process holds: inside it (launches.concurrent == 2) neither the tail split nor the side path engages, although its sub-batches have
    32 rows and the model knows the shape, and _whole_seen is not written."""
    import lemevit_amd.model as M
    from lemevit_amd.graph import split_forward

    class Watched(dict):
        writes = 0

        def __setitem__(self, k, v):
            Watched.writes += 1
            super().__setitem__(k, v)

    m, spy, aux = _model("lemevit_tiny"), _SplitSpy(monkeypatch), _AuxSpy(monkeypatch)
    _fwd(m, _image(224, 32))          # the shape is known: a pass with launches.concurrent == 1 WOULD split from here on
    key, seen = _seen(m)
    assert seen[3] and not seen[4]
    m._whole_seen = Watched(m._whole_seen)
    aux.take()
    img = _image(224, 64)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        y1 = split_forward(m, img, 2)
        y2 = split_forward(m, img, 2)
    torch.cuda.synchronize()
    assert spy.take() == []
    assert aux.take() == [1, 1], "only split_forward itself may fork (one auxiliary stream per call)"
    assert Watched.writes == 0 and dict(m._whole_seen) == {key: seen}
    assert M.launches.concurrent == 1
    assert torch.equal(y1, y2)
    _fwd(m, _image(224, 32))          # (and the watch itself sees an ordinary pass)
    assert Watched.writes == 1 and len(spy.take()) == 1


# ---- 8. the concurrency claim inside the tail ------------------------------------------------------------------------------------------------------------------------------------------
def test_tail_sub_batches_claim_their_concurrency(monkeypatch):
    """_tail_split trusts the PREVIOUS pass's record of which stages ran as persistent launches.  With a stale record (here: written by hand, so that the split starts
    one stage early, at the "S" stage 3 of LeMeViT-Tiny) a stage inside the tail is eligible for a persistent kernel, and `parts` launches of it would run side by side: _sstage_applies
    and the ops must then see launches.concurrent == parts -- the claim lmv_*stage_max_concurrent judges -- not 1.  The recorder answers None for every call from inside the tail, so no
    persistent kernel is launched in the contested state, with or without the fix.  launches.concurrent is back to 1 afterwards, also when a sub-batch raises.
    (Before the fix the recorded values were 1.)"""
    import lemevit_amd.model as M
    m, img, spy = _model("lemevit_tiny"), _image(224, 32), _SplitSpy(monkeypatch)
    p1 = _fwd(m, img)
    key, seen = _seen(m)
    assert seen[3] and not seen[4]
    stale = tuple(j == 2 for j in range(len(seen)))          # "stage 2 was the last persistent launch": the tail starts at stage 3
    recorded, orig_applies = [], M._sstage_applies

    def applies(stage, xt, c, H, W):
        if spy.inside:
            recorded.append((M.launches.concurrent, xt.shape[0], orig_applies(stage, xt, c, H, W)))
            return None
        return orig_applies(stage, xt, c, H, W)

    monkeypatch.setattr(M, "_sstage_applies", applies)
    try:
        m._whole_seen[key] = stale
        y = _fwd(m, img)
        torch.cuda.synchronize()
        calls = spy.take()
        assert [(c["stage"], c["rows"], c["concurrent"]) for c in calls] == [(3, [16, 16], 1)], calls
        assert len(recorded) == 4, recorded          # stages 3 and 4 of two sub-batches
        assert all(n == 2 and rows == 16 for n, rows, _ in recorded), f"launches.concurrent inside the tail (concurrent, rows, verdict): {recorded}"
        assert M.launches.concurrent == 1
        close(y, p1, BF16_E2E, "stage 3 on the per-block schedule inside the tail vs pass 1")

        # a sub-batch that raises: the claim is withdrawn on the way out
        m._whole_seen[key] = stale
        orig_from, subs = M.LeMeViT._stages_from, []

        def stages_from(model, i0, x, xt, H, W, c, hoist, st):
            if spy.inside:
                subs.append(M.launches.concurrent)
                if len(subs) == 2:
                    raise RuntimeError("forced: second sub-batch")
            return orig_from(model, i0, x, xt, H, W, c, hoist, st)

        monkeypatch.setattr(M.LeMeViT, "_stages_from", stages_from)
        with pytest.raises(RuntimeError, match="forced: second sub-batch"):
            _fwd(m, img)
        torch.cuda.synchronize()
        assert len(spy.take()) == 1 and subs == [2, 2], subs
        assert M.launches.concurrent == 1
        assert spy.inside == 0 and torch.cuda.current_stream() == torch.cuda.default_stream()
    finally:
        M.launches.concurrent = 1
