"""CPU: the host state between a weight-gradient launch and the ``.grad`` (or gradient-bucket view) the optimiser reads -- the route
``ops._wg_route`` picks per layer, the five scoping context managers, what ``weight_grads_on_side_stream().join()`` settles, and the
single-rank state machines of ``ops.ReplayedChain`` / ``ops.ReplayedPrepack`` (a recorder stands in for the HIP capture, as in
tests/test_ddp_gloo.py, which covers the gated two-rank case).  Nothing here launches a kernel: routing, hand-over and the replay
policies are host decisions, taken before (or instead of) any launch."""
import warnings

import pytest
import torch

from vibravox_amd import ops


class Sink:
    """``ddp.GradSync`` as the hand-over sees it: a gradient-bucket view per parameter it knows, and the report."""

    def __init__(self, params, watch=()):
        self.views = {id(p): torch.zeros_like(p) for p in params}
        self.ready, self.watch, self.grads_seen = [], list(watch), []

    def grad_buffer(self, p):
        return self.views.get(id(p))

    def mark_ready(self, ps):
        self.ready.append(list(ps))
        self.grads_seen.append([p.grad for p in self.watch])


def layer(bias: bool = True, gain: bool = True):
    """(v, g, bias) of a weight-normalised conv of 4 output channels."""
    torch.manual_seed(0)
    v = torch.nn.Parameter(torch.randn(4, 3, 5))
    g = torch.nn.Parameter(torch.randn(4, 1, 1)) if gain else None
    b = torch.nn.Parameter(torch.randn(4)) if bias else None
    return v, g, b


def check_fresh(params, outs, *sinks):
    for p, o in zip(params, outs):
        if p is None:
            assert o is None
            continue
        assert tuple(o.shape) == ((params[0].shape[0],) if p is params[2] else tuple(p.shape)) and o.dtype is torch.float32
        assert o is not p.grad and all(o is not view for s in sinks for view in s.views.values())


def check_views(params, outs, sink):
    for p, o in zip(params, outs):
        assert (o is None) if p is None else (o is sink.views[id(p)])


def found(cm, field: str):
    """What a scoping context manager found on entry (its ``prev``): the value itself, or the field of the record it saved."""
    with cm:
        pass
    return getattr(cm.prev, field, cm.prev)


def observed_mode():
    """(input gradients skipped, weight gradients skipped, backward arithmetic), each as a fresh ``with`` finds it."""
    return (found(ops.input_grads_disabled(), "skip_input_grads"), found(ops.weight_grads_disabled(), "skip_weight_grads"),
            found(ops.backward_math(ops.MATH_BF16), "math"))


# ---- 1. the routing table ------------------------------------------------------------------------------------------------------------
def test_no_scope_launches_now_into_fresh_tensors():
    for params in (layer(), layer(bias=False), layer(bias=False, gain=False)):
        use_side, outs, sunk = ops._wg_route(*params)
        assert (use_side, sunk) == (False, False)
        check_fresh(params, outs)
    v, g, b = layer()
    v.grad = torch.ones_like(v)
    use_side, outs, sunk = ops._wg_route(v, g, b)
    assert (use_side, sunk) == (False, False)
    check_fresh((v, g, b), outs)


def test_side_scope_without_a_sink_defers_layers_that_hold_no_gradient_and_no_hook():
    with ops.weight_grads_on_side_stream():
        for params in (layer(), layer(bias=False), layer(bias=False, gain=False)):
            use_side, outs, sunk = ops._wg_route(*params)
            assert (use_side, sunk) == (True, False)
            check_fresh(params, outs)
        for held in range(3):   # one of v / g / bias holds a gradient: the whole layer goes through autograd
            params = layer()
            params[held].grad = torch.ones_like(params[held])
            use_side, outs, sunk = ops._wg_route(*params)
            assert (use_side, sunk) == (False, False)
            check_fresh(params, outs)
        for hooked in range(3):
            for register in ("register_post_accumulate_grad_hook", "register_hook"):
                params = layer()
                getattr(params[hooked], register)(lambda *a: None)
                use_side, outs, sunk = ops._wg_route(*params)
                assert (use_side, sunk) == (False, False)
                check_fresh(params, outs)
        use_side, _, sunk = ops._wg_route(torch.randn(4, 3, 5), None, None)   # a plain tensor is nobody's ``.grad`` to assign
        assert (use_side, sunk) == (False, False)


def test_collecting_inside_a_side_scope_without_a_sink_launches_now():
    jobs = []
    with ops.weight_grads_on_side_stream():
        with ops.collect_wn_jobs(jobs):
            for params in (layer(), layer(bias=False, gain=False)):
                use_side, outs, sunk = ops._wg_route(*params)
                assert (use_side, sunk) == (False, False)
                check_fresh(params, outs)
        assert ops._wg_route(*layer())[0] is True   # the side route is back
    assert jobs == []   # routing appends nothing: ``_wg_finish`` does


def test_side_scope_with_a_sink_writes_into_its_views():
    for params in (layer(), layer(bias=False), layer(bias=False, gain=False)):
        sink = Sink([p for p in params if p is not None])
        for p in params:
            if p is not None:
                p.grad = sink.views[id(p)]   # data-parallel: every .grad IS its bucket view, so "holds no gradient" never applies
        with ops.weight_grads_on_side_stream(sink):
            use_side, outs, sunk = ops._wg_route(*params)
            assert (use_side, sunk) == (True, True)
            check_views(params, outs, sink)
            with ops.collect_wn_jobs([], sink):   # the graph-captured body: same views, launched on the caller's stream
                use_side, outs, sunk = ops._wg_route(*params)
                assert (use_side, sunk) == (False, True)
                check_views(params, outs, sink)
            use_side, outs, sunk = ops._wg_route(*params)
            assert (use_side, sunk) == (True, True)
        assert sink.ready == []
        use_side, outs, sunk = ops._wg_route(*params)   # outside: no sink
        assert (use_side, sunk) == (False, False)
        check_fresh(params, outs, sink)


def test_a_sink_that_lacks_one_buffer_is_not_used_for_that_layer():
    for missing in range(3):
        params = layer()
        sink = Sink([p for i, p in enumerate(params) if i != missing])
        for i, p in enumerate(params):
            if i != missing:
                p.grad = sink.views[id(p)]
        with ops.weight_grads_on_side_stream(sink):
            use_side, outs, sunk = ops._wg_route(*params)
            assert (use_side, sunk) == (False, False)
            check_fresh(params, outs, sink)   # whole-layer rule: not even the buffers it has


# ---- 2. scope restoration ------------------------------------------------------------------------------------------------------------
def test_five_nested_scopes_unwind_through_an_exception():
    assert observed_mode() == (False, False, ops.MATH_F32)
    params = layer()
    sink = Sink(params)
    for p in params:
        p.grad = sink.views[id(p)]
    jobs = []
    with pytest.raises(KeyError):
        with ops.weight_grads_on_side_stream(sink):
            with ops.collect_wn_jobs(jobs, sink):
                with ops.backward_math(ops.MATH_BF16):
                    with ops.input_grads_disabled():
                        with ops.weight_grads_disabled():
                            assert observed_mode() == (True, True, ops.MATH_BF16)
                            assert ops._wg_route(*params)[::2] == (False, True)
                            raise KeyError("inside the innermost scope")
    assert observed_mode() == (False, False, ops.MATH_F32)
    use_side, outs, sunk = ops._wg_route(*params)
    assert (use_side, sunk) == (False, False)
    check_fresh(params, outs, sink)
    with ops.backward_math(ops.MATH_BF16):   # each scope restores what it found, not the default
        with ops.backward_math(ops.MATH_BF16X3):
            pass
        assert observed_mode() == (False, False, ops.MATH_BF16)
    assert jobs == [] and sink.ready == []


# ---- 3. the join ---------------------------------------------------------------------------------------------------------------------
def job_of(params, outs):
    v, g, _ = params
    return ops.wn_job(torch.zeros(2 * v.numel()), 2, v.numel() // v.shape[0], v, g, None if g is None else torch.ones(v.shape[0]), outs)


def test_join_assigns_accumulates_and_reports_once():
    """On a CPU no side stream exists (``aux_stream`` is never asked), so ``join()`` does not reach the slab-sum launch: the outputs
    hold what this test wrote into them.  What is checked is the hand-over behind that launch."""
    a, b = layer(), layer(bias=False)
    sink = Sink([p for p in b if p is not None], watch=[a[0], a[1], a[2]])
    for p in b[:2]:
        p.grad = sink.views[id(p)]
    held = a[1].grad = torch.ones_like(a[1])   # not what _wg_route would defer: _wg_finish assigns or accumulates whatever it is handed
    with ops.weight_grads_on_side_stream(sink) as side:
        outs_a, _ = ops.grad_outputs(*a)
        for o in outs_a:
            o.fill_(2.0)
        outs_b, sunk_b = ops.grad_outputs(*b, sink, whole_layer=True)
        assert sunk_b
        keep = (torch.zeros(3),)
        res = ops._wg_finish(True, keep, [(job_of(a, outs_a), a, False), (job_of(b, outs_b), b, True)])
        assert res == [(None, None, None)] * 2
        assert a[0].grad is None and sink.ready == []   # nothing before the join
        side.join()
    assert a[0].grad is outs_a[0] and a[2].grad is outs_a[2]
    assert a[1].grad is held and torch.equal(held, torch.full_like(held, 3.0))
    assert len(sink.ready) == 1 and [id(p) for p in sink.ready[0]] == [id(p) for p in b[:2]]
    assert sink.grads_seen[0][0] is outs_a[0] and sink.grads_seen[0][2] is outs_a[2]   # reported after the assignments
    side.join()   # a second join owes nothing
    assert len(sink.ready) == 1 and torch.equal(held, torch.full_like(held, 3.0)) and a[0].grad is outs_a[0]


def test_an_exception_inside_the_side_scope_leaves_nothing_to_join():
    a, b = layer(), layer(bias=False)
    sink = Sink([p for p in b if p is not None])
    outs_a, _ = ops.grad_outputs(*a)
    outs_b, _ = ops.grad_outputs(*b, sink, whole_layer=True)
    with pytest.raises(KeyError):
        with ops.weight_grads_on_side_stream(sink):
            ops._wg_finish(True, (torch.zeros(3),), [(job_of(a, outs_a), a, False), (job_of(b, outs_b), b, True)])
            raise KeyError("backward failed half-way")
    with ops.weight_grads_on_side_stream(sink) as side:
        side.join()
    assert all(p.grad is None for p in a) and sink.ready == []


def test_the_immediate_route_of_wg_finish_collects_or_returns_the_outputs():
    a = layer()
    outs, _ = ops.grad_outputs(*a)
    job, jobs = job_of(a, outs), []
    with ops.collect_wn_jobs(jobs):
        res = ops._wg_finish(False, (), [(job, a, False)])
    assert jobs == [job] and all(r is o for r, o in zip(res[0], outs))


# ---- 4. the replayers, single rank ---------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for both ``_capture`` methods; ``log`` holds eager / capture / replay events in program order."""

    def __init__(self):
        self.log, self.fail = [], set()
        self.saved = (ops.ReplayedChain._capture, ops.ReplayedPrepack._capture, ops.ReplayedChain.enabled, ops.ReplayedPrepack.enabled)
        ops.ReplayedChain._capture = staticmethod(self.chain_capture)
        ops.ReplayedPrepack._capture = staticmethod(self.prepack_capture)
        ops.ReplayedChain.enabled = ops.ReplayedPrepack.enabled = True

    def restore(self):
        chain, prepack, ops.ReplayedChain.enabled, ops.ReplayedPrepack.enabled = self.saved
        ops.ReplayedChain._capture, ops.ReplayedPrepack._capture = staticmethod(chain), staticmethod(prepack)

    class Graph:
        def __init__(self, log, name):
            self.log, self.name = log, name

        def replay(self):
            self.log.append("replay " + self.name)

    def chain_capture(self, fn, stream_):
        if "chain" in self.fail:
            raise RuntimeError("no capture today")
        self.capturing = True
        try:
            out = fn()
        finally:
            self.capturing = False
        return Recorder.Graph(self.log, out[0]), out

    def prepack_capture(self, body, stream_):
        if "prepack" in self.fail:
            raise RuntimeError("no capture today")
        self.capturing = True
        try:
            body()
        finally:
            self.capturing = False
        return Recorder.Graph(self.log, "prepack")

    capturing = False

    def body(self, name):
        def fn():
            self.log.append(("capture " if self.capturing else "eager ") + name)
            return (name, object())   # a fresh result per run, like tensors of an eager call
        return fn

    def take(self):
        log, self.log[:] = list(self.log), []
        return log


@pytest.fixture
def rec():
    r = Recorder()
    try:
        yield r
    finally:
        r.restore()


def test_chain_with_a_constant_signature(rec):
    pending, captured = ops.graphs_pending(), ops.graphs_captured()
    chain = ops.ReplayedChain()
    assert (ops.graphs_pending(), ops.graphs_captured()) == (pending, captured)   # no signature yet: not in use
    first = chain.run("A", rec.body("A"), None)
    assert rec.take() == ["eager A"] and chain.graph is None
    assert (ops.graphs_pending(), ops.graphs_captured()) == (pending + 1, captured)
    out = chain.run("A", rec.body("A"), None)
    assert rec.take() == ["capture A", "replay A"] and out is not first
    assert (ops.graphs_pending(), ops.graphs_captured()) == (pending, captured + 1)
    assert chain.graph is not None and chain.sig == "A" and chain.out is out and chain.captures > 0
    for _ in range(3):
        assert chain.run("A", rec.body("A"), None) is out   # the captured object, rewritten in place by a real replay
        assert rec.take() == ["replay A"]
    del chain
    assert ops.graphs_captured() == captured


def test_chain_with_alternating_signatures(rec):
    chain = ops.ReplayedChain()
    outs = {}
    for k, want in enumerate((["eager A"], ["eager B"], ["capture A", "replay A"], ["capture B", "replay B"])):
        sig = "AB"[k % 2]
        outs[sig] = chain.run(sig, rec.body(sig), None)
        assert rec.take() == want
    generation = {}
    for k in range(4):
        sig = "AB"[k % 2]
        assert chain.run(sig, rec.body(sig), None) is outs[sig] and rec.take() == ["replay " + sig]
        assert chain.sig == sig and chain.out is outs[sig]
        assert generation.setdefault(sig, chain.captures) == chain.captures
    assert generation["A"] != generation["B"]


def test_chain_keeps_the_most_recent_graphs_and_recaptures_an_evicted_one(rec):
    keep = max(1, ops.ReplayedChain.KEEP)
    sigs = [f"s{i}" for i in range(keep + 1)]
    chain = ops.ReplayedChain()
    for s in sigs:
        chain.run(s, rec.body(s), None)
        assert rec.take() == ["eager " + s]
    outs, generation = {}, {}
    for s in sigs:
        outs[s] = chain.run(s, rec.body(s), None)
        generation[s] = chain.captures
        assert rec.take() == ["capture " + s, "replay " + s]   # all are captured
    assert len(set(generation.values())) == len(sigs)
    for s in sigs[1:]:   # the most recent KEEP are cache hits, and ``captures`` names the hit's generation again
        assert chain.run(s, rec.body(s), None) is outs[s] and rec.take() == ["replay " + s]
        assert chain.captures == generation[s]
    oldest = sigs[0]   # evicted by the last capture: one eager round, then captured again
    chain.run(oldest, rec.body(oldest), None)
    assert rec.take() == ["eager " + oldest] and chain.graph is None and chain.out is None
    again = chain.run(oldest, rec.body(oldest), None)
    assert rec.take() == ["capture " + oldest, "replay " + oldest]
    assert again is not outs[oldest] and chain.captures not in generation.values()
    assert chain.run(sigs[-1], rec.body(sigs[-1]), None) is outs[sigs[-1]] and chain.captures == generation[sigs[-1]]
    assert rec.take() == ["replay " + sigs[-1]]


def test_prepack_with_a_constant_signature(rec):
    pending, captured = ops.graphs_pending(), ops.graphs_captured()
    pre = ops.ReplayedPrepack()
    assert pre.run("A", rec.body("A"), None) is False and rec.take() == ["eager A"]
    assert (ops.graphs_pending(), ops.graphs_captured()) == (pending + 1, captured)
    assert pre.run("A", rec.body("A"), None) is False and rec.take() == ["eager A"]
    assert (ops.graphs_pending(), ops.graphs_captured()) == (pending + 1, captured)
    assert pre.run("A", rec.body("A"), None) is False   # the body ran, under capture: its bookkeeping is current
    assert rec.take() == ["capture A", "replay prepack"]
    assert (ops.graphs_pending(), ops.graphs_captured()) == (pending, captured + 1)
    for _ in range(2):
        assert pre.run("A", rec.body("A"), None) is True and rec.take() == ["replay prepack"]
    assert pre.graph is not None and pre.sig == "A"


def test_prepack_with_alternating_signatures_is_never_captured(rec):
    pre = ops.ReplayedPrepack()
    for k in range(10):
        sig = "AB"[k % 2]
        assert pre.run(sig, rec.body(sig), None) is False and rec.take() == ["eager " + sig]
    assert pre.graph is None


def test_prepack_drops_its_graph_on_another_signature(rec):
    pre = ops.ReplayedPrepack()
    for _ in range(4):
        pre.run("A", rec.body("A"), None)
    assert rec.take() == ["eager A", "eager A", "capture A", "replay prepack", "replay prepack"]
    assert pre.run("B", rec.body("B"), None) is False and rec.take() == ["eager B"] and pre.graph is None
    results = [pre.run("A", rec.body("A"), None) for _ in range(4)]   # its three rounds again
    assert results == [False, False, False, True]
    assert rec.take() == ["eager A", "eager A", "capture A", "replay prepack", "replay prepack"]


@pytest.mark.parametrize("failing", ["chain", "prepack"])
def test_a_failed_capture_leaves_that_class_eager_and_the_other_alone(rec, failing):
    rec.fail.add(failing)
    chain, pre = ops.ReplayedChain(), ops.ReplayedPrepack()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        chain_log = []
        for _ in range(4):
            chain.run("A", rec.body("A"), None)
            chain_log.append(rec.take())
        pre_log = []
        for _ in range(5):
            pre.run("A", rec.body("A"), None)
            pre_log.append(rec.take())
    assert len(caught) == 1 and f"{failing} graph capture failed" in str(caught[0].message)
    if failing == "chain":
        assert chain_log == [["eager A"]] * 4 and chain.graph is None   # once per call, the failing one included
        assert ops.ReplayedChain.enabled is False and ops.ReplayedPrepack.enabled is True
        assert pre_log == [["eager A"], ["eager A"], ["capture A", "replay prepack"], ["replay prepack"], ["replay prepack"]]
    else:
        assert pre_log == [["eager A"]] * 5 and pre.graph is None
        assert ops.ReplayedPrepack.enabled is False and ops.ReplayedChain.enabled is True
        assert chain_log == [["eager A"], ["capture A", "replay A"], ["replay A"], ["replay A"]]


# ---- 5. the typed records (new with them) --------------------------------------------------------------------------------------------
def test_a_misspelt_field_is_an_error():
    mode, pending = ops._mode, ops._pending
    assert mode.sink is None and pending.assign == []
    with pytest.raises(AttributeError):
        mode.sinc = None
    with pytest.raises(AttributeError):
        mode.sink = None   # immutable: scopes replace the record
    with pytest.raises(AttributeError):
        pending.asign = []
    with pytest.raises(ValueError):
        mode._replace(sinc=None)
