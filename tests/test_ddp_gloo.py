"""CPU, world_size 2, gloo: the data-parallel gradient exchange (vibravox_amd/ddp.py) that bench.py
uses with RCCL on the GPUs -- bucketed all-reduce with gradients living in the bucket buffers,
launched from post-accumulate hooks, averaged by the optimizer's grad_scale."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vibravox_amd.ddp import BucketedZeroGrad, GradSync, all_reduce_scalars

        torch.manual_seed(0)  # identical weights on both ranks
        net = torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
        ref = torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
        ref.load_state_dict(net.state_dict())
        sync = GradSync(net.parameters(), bucket_bytes=600)  # forces several buckets
        assert len(sync.buckets) >= 3
        opt = BucketedZeroGrad(torch.optim.SGD(net.parameters(), lr=0.1), sync)
        ref_opt = torch.optim.SGD(ref.parameters(), lr=0.1)
        g = torch.Generator().manual_seed(100)
        data = torch.randn(2, 4, 7, generator=g)  # same on both ranks; rank r trains on data[r]
        for step in range(3):
            x = data[rank] + step
            net(x).pow(2).sum().backward()
            scale = sync.finish()
            assert scale == 1.0 / world
            for p in net.parameters():
                p.grad.mul_(scale)
            opt.step()
            opt.zero_grad()
            # single-process reference: mean of the per-rank gradients
            ref_opt.zero_grad()
            sum(ref(data[r] + step).pow(2).sum() for r in range(world)).backward()
            for p in ref.parameters():
                p.grad.div_(world)
            ref_opt.step()
            for p, r in zip(net.parameters(), ref.parameters()):
                assert torch.allclose(p, r, atol=1e-6), (step, (p - r).abs().max())
            assert all(p.grad is v for b in sync.buckets for p, v in zip(b.params, b.views))  # grads stay bucket views
        assert sync.launched >= 3 * len(sync.buckets)  # every bucket went out from its hook, every step
        # the sink form the engine step uses: gradients computed outside autograd are written straight into the bucket views
        # (grad_buffer) and reported with mark_ready -- same exchange, same result
        launched = sync.launched
        x = data[rank] + 7
        grads = torch.autograd.grad(net(x).pow(2).sum(), list(net.parameters()))
        plist = list(net.parameters())
        for p, gr in zip(plist, grads):
            buf = sync.grad_buffer(p)
            assert buf is not None and buf.shape == p.shape and buf.is_contiguous()
            buf.copy_(gr)
        sync.mark_ready(reversed(plist))
        scale = sync.finish()
        assert sync.launched == launched + len(sync.buckets)
        want = torch.autograd.grad(sum(ref(data[r] + 7).pow(2).sum() for r in range(world)), list(ref.parameters()))
        for p, w in zip(plist, want):
            assert p.grad is sync.grad_buffer(p)
            assert torch.allclose(p.grad * scale, w / world, atol=1e-6)
        opt.zero_grad()
        vals = all_reduce_scalars([torch.tensor(float(rank)), torch.tensor(10.0 + rank)])
        assert abs(float(vals[0]) - 0.5) < 1e-6 and abs(float(vals[1]) - 10.5) < 1e-6
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        q.put((rank, f"{type(e).__name__}: {e}"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_bucketed_gradient_allreduce_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=100) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


def _engine_sequence_worker(rank, world, port, q):
    """The data-parallel call sequence of the engine train step (lightning_modules/eben.py: ``_training_step_engine``, whose phases ``_engine_generator_update`` /
    ``_engine_discriminator_update`` hand ``_grad_sink(optimizer)`` to the backward and end in ``_finish(optimizer)``) on CPU
    tensors: TWO GradSyncs; the generator's gradients partly through autograd's hooks and partly through the sink
    (grad_buffer + mark_ready at the side-stream join); the discriminator's written into the bucket views chain by chain,
    the LAST chain first (disc_engine.backward_finish), each chain reported by its own mark_ready; finish() + the
    optimiser's grad_scale; the step's sync_dist values reduced by ONE packed collective (base_se.flush_logged)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vibravox_amd.ddp import BucketedZeroGrad, GradSync
        from vibravox_amd.lightning_modules.base_se import BaseSELightningModule

        torch.manual_seed(0)
        gen = torch.nn.Sequential(torch.nn.Linear(6, 20), torch.nn.Tanh(), torch.nn.Linear(20, 4))
        chains = [torch.nn.Sequential(torch.nn.Linear(4, 9), torch.nn.Tanh(), torch.nn.Linear(9, 1)) for _ in range(3)]
        disc = torch.nn.ModuleList(chains)
        g_sync, d_sync = GradSync(gen.parameters(), bucket_bytes=300), GradSync(disc.parameters(), bucket_bytes=200)
        assert len(g_sync.buckets) >= 2 and len(d_sync.buckets) >= 3
        # a discriminator bucket that straddles two chains must wait for both reports
        owners = [{id(p) for p in ch.parameters()} for ch in chains]
        assert any(sum(any(id(p) in o for p in b.params) for o in owners) > 1 for b in d_sync.buckets)
        g_opt = BucketedZeroGrad(torch.optim.SGD(gen.parameters(), lr=0.1), g_sync)
        d_opt = BucketedZeroGrad(torch.optim.SGD(disc.parameters(), lr=0.1), d_sync)
        data = torch.randn(world, 5, 6, generator=torch.Generator().manual_seed(3))
        mod = BaseSELightningModule(sample_rate=16000)
        for step in range(2):
            x = data[rank] + step
            fake = gen(x)
            # ---- discriminator gradients "outside autograd", written into the bucket views, last chain first
            d_loss = sum(ch(fake.detach()).pow(2).mean() for ch in chains)
            grads = torch.autograd.grad(d_loss, list(disc.parameters()))
            by_param = {id(p): g for p, g in zip(disc.parameters(), grads)}
            launched_before = d_sync.launched
            for ci in (2, 0, 1):
                plist = list(chains[ci].parameters())
                for p in plist:
                    d_sync.grad_buffer(p).copy_(by_param[id(p)])
                d_sync.mark_ready(plist)
                if ci == 2:   # only buckets that the last chain fills on its own can have left yet
                    gone = d_sync.order[len(d_sync.order) - (d_sync.launched - launched_before):] if d_sync.launched > launched_before else []
                    assert all(id(p) in owners[2] for i in gone for p in d_sync.buckets[i].params)
            # ---- generator: first layer through the sink (side-stream join), the rest through autograd's hooks
            g_loss = sum(ch(fake).mean() for ch in chains)
            first = list(gen[0].parameters())
            rest = [p for p in gen.parameters() if all(p is not f for f in first)]
            g_first = torch.autograd.grad(g_loss, first, retain_graph=True)
            torch.autograd.backward(g_loss, inputs=rest)
            for p, g in zip(first, g_first):
                g_sync.grad_buffer(p).copy_(g)
            g_sync.mark_ready(first)
            mod.log("train/generator/x", g_loss.detach(), sync_dist=True)
            mod.log("train/discriminator/y", d_loss.detach(), sync_dist=True)
            g_scale, d_scale = g_sync.finish(), d_sync.finish()
            assert g_scale == d_scale == 1.0 / world
            # reference: the mean over ranks of the per-rank gradients, computed locally from every rank's data
            ref_g = [torch.zeros_like(p) for p in gen.parameters()]
            ref_d = [torch.zeros_like(p) for p in disc.parameters()]
            ref_losses = [0.0, 0.0]
            for r in range(world):
                f = gen(data[r] + step)
                dl = sum(ch(f.detach()).pow(2).mean() for ch in chains)
                gl = sum(ch(f).mean() for ch in chains)
                for acc, g in zip(ref_d, torch.autograd.grad(dl, list(disc.parameters()))):
                    acc += g / world
                for acc, g in zip(ref_g, torch.autograd.grad(gl, list(gen.parameters()))):
                    acc += g / world
                ref_losses[0] += float(gl) / world
                ref_losses[1] += float(dl) / world
            for p, want in zip(gen.parameters(), ref_g):
                assert torch.allclose(p.grad * g_scale, want, atol=1e-6)
            for p, want in zip(disc.parameters(), ref_d):
                assert p.grad is d_sync.grad_buffer(p) and torch.allclose(p.grad * d_scale, want, atol=1e-6)
            for opt, scale in ((g_opt, g_scale), (d_opt, d_scale)):
                for grp in opt.param_groups:
                    for p in grp["params"]:
                        p.grad.mul_(scale)
                opt.step()
                opt.zero_grad()
            # the packed scalar reduction: local values until the flush, rank means after it
            assert abs(float(mod.logged["train/generator/x"]) - float(g_loss)) < 1e-7
            mod.flush_logged()
            assert abs(float(mod.logged["train/generator/x"]) - ref_losses[0]) < 1e-6
            assert abs(float(mod.logged["train/discriminator/y"]) - ref_losses[1]) < 1e-6
            assert mod._sync_pending == []
        # deterministic exchange order: every rank issued the same buckets in the same order
        mine = torch.tensor(d_sync.order + [-1] + g_sync.order)
        both = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        assert all(torch.equal(both[0], o) for o in both)
        assert len(d_sync.order) == 2 * len(d_sync.buckets) and len(g_sync.order) == 2 * len(g_sync.buckets)
        # replicas stayed identical
        flat = torch.cat([p.detach().flatten() for p in list(gen.parameters()) + list(disc.parameters())])
        other = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(other, flat)
        assert all(torch.equal(other[0], o) for o in other)
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_engine_step_exchange_sequence_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_engine_sequence_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=100) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


# ---- multi-rank graph captures: the ranks agree on the step (ops.CaptureGate) ---------------------------------------------------------
def _capture_gate_worker(rank, world, port, q):
    """Drives the state machines of ``ops.ReplayedChain`` / ``ops.ReplayedPrepack`` over 16 steps of a mock train step -- a forward chain,
    a backward chain whose signature contains the forward's output address (it settles one level later, like the engine's), a prepack --
    with a recorder in place of the HIP capture and gloo all-reduces as the gradient buckets.  Rank 1's allocator history differs: its
    forward sees a one-off signature in step 1, so that WITHOUT the gate its captures would land one step after rank 0's."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vibravox_amd import ops

        gate = ops.capture_gate
        gate.reset()
        assert gate.active()
        log = []          # (step, event) in program order: captures and collectives
        inflight = [0]    # collectives issued and not yet waited for
        step = [0]

        class FakeGraph:
            def __init__(self, name):
                self.name = name

            def replay(self):
                log.append((step[0], "replay " + self.name))

        def fake_chain_capture(fn, stream_):
            assert inflight[0] == 0, "a capture started while a bucket's collective was in flight"
            out = fn()
            log.append((step[0], "capture chain " + out[0]))
            return FakeGraph(out[0]), out

        def fake_prepack_capture(body, stream_):
            assert inflight[0] == 0, "a capture started while a bucket's collective was in flight"
            body()
            log.append((step[0], "capture prepack"))
            return FakeGraph("prepack")

        ops.ReplayedChain._capture = staticmethod(fake_chain_capture)
        ops.ReplayedPrepack._capture = staticmethod(fake_prepack_capture)
        ops.ReplayedChain.enabled = ops.ReplayedPrepack.enabled = True
        works = []

        def drain():
            for w in works:
                w.wait()
            works.clear()
            inflight[0] = 0

        gate.register_drain(drain)
        fwd, bwd, pre = ops.ReplayedChain(), ops.ReplayedChain(), ops.ReplayedPrepack()
        bucket = [torch.ones(4) * (rank + 1) for _ in range(2)]
        for s in range(16):
            step[0] = s
            # forward: rank 1's signature is different ONCE (an allocation that moved)
            fsig = ("fwd", 1000 + (7 if (rank == 1 and s == 1) else 0))
            out = fwd.run(fsig, lambda: ("fwd", 0x5000 if fwd.graph is None else 0x9000), None)
            # backward: reads the forward's output (its address changes once the forward replays from its pool)
            addr = 0x9000 if fwd.graph is not None else 0x5000 + s   # eager outputs move around, pooled ones do not
            bwd.run(("bwd", addr), lambda: ("bwd", 0), None)
            # gradient buckets: issued asynchronously, waited for in front of "Adam"
            for b in bucket:
                works.append(dist.all_reduce(b, op=dist.ReduceOp.SUM, async_op=True))
                inflight[0] += 1
                log.append((s, "allreduce"))
            pre.run(("prepack", 1), lambda: None, None)   # rebuilds the weight images while the exchange is in flight
            drain()
            gate.step_end()
        captures = [e for e in log if e[1].startswith("capture")]
        assert {c[1] for c in captures} == {"capture chain fwd", "capture chain bwd", "capture prepack"}, captures
        assert gate.settled and not gate.open
        assert fwd.graph is not None and bwd.graph is not None and pre.graph is not None
        assert ops.graphs_pending() == 0
        q.put((rank, "ok", captures, [e for e in gate.history], [e for e in log if e[1] == "allreduce"]))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}", None, None, None))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_graph_captures_happen_in_the_same_step_on_both_ranks():
    """ops.CaptureGate: identical capture steps, identical vote history and identical collective order on the two ranks although rank 1's
    signatures settle one step later; no capture while a collective is in flight (asserted inside the recorder)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_capture_gate_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=100) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=30)
    assert [r[1] for r in results] == ["ok", "ok"], results
    (_, _, cap0, hist0, coll0), (_, _, cap1, hist1, coll1) = results
    assert cap0 == cap1 and len(cap0) == 3          # same sequences captured in the same steps
    assert hist0 == hist1                           # same votes, same outcome, settled in the same step
    assert coll0 == coll1 and len(coll0) == 32      # the collectives' program order never depended on the captures
