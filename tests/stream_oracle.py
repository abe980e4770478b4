"""Test-side restatement of the streaming generator (TEST INFRASTRUCTURE): plain float64 torch, layer by layer over the oracle's weights,
executing the operations of a ``vibravox_amd.streaming.Schedule`` push by push.

Every layer here applies its edge rule at both ends of its BUFFER, as the device kernels do.  The state buffers are as long as the
plan's capacities and hold NaN everywhere outside ``[carry | new]``; every output of a layer outside the range the schedule declares
exact is overwritten with NaN as well.  A sample can therefore only come out right if the schedule's carries, offsets and frontiers
are right: whatever reads junk, or a sample that was never delivered, reads NaN.
"""
import torch
import torch.nn.functional as F

from oracle import eben_oracle as O
from vibravox_amd import streaming

NAN = float("nan")


class OracleStream:
    def __init__(self, gen, sd, chunk_samples, rows=1):
        self.gen, self.sd, self.rows = gen, sd, rows
        self.plan = streaming.plan(gen, chunk_samples)
        self.schedule = streaming.Schedule(gen, chunk_samples)
        self.nodes = self.schedule.by_name
        self.bufs = {t.name: [torch.full((rows, t.channels, t.capacity), NAN, dtype=torch.float64) for _ in range(2)] for t in self.plan.tensors}
        self.cur = {t.name: 0 for t in self.plan.tensors}
        self.length = {t.name: 0 for t in self.plan.tensors}
        self.out = {}
        self.longest = {t.name: 0 for t in self.plan.tensors}   # the longest buffer seen per tensor, for the capacity check

    # ---- operands ---------------------------------------------------------------------------------------------------------------------
    def _read(self, name, chunk):
        """(tensor, its length) -- a state buffer is returned whole, poison included."""
        if name == "input":
            return chunk, chunk.shape[2]
        kind, key = name.split(":", 1)
        if kind == "out":
            return self.out[key], self.out[key].shape[2]
        return self.bufs[key][self.cur[key]], self.length[key]

    def _splice(self, op, chunk, emitted):
        parts = []
        if op.n_carry:
            prev, n = self._read(op.prev, chunk)
            assert 0 <= op.prev_off and op.prev_off + op.n_carry <= n, op
            parts.append(prev[:, :, op.prev_off : op.prev_off + op.n_carry])
        if op.n_new:
            src, n = self._read(op.src, chunk)
            assert 0 <= op.src_off and op.src_off + op.n_new <= n, op
            new = src[:, :, op.src_off : op.src_off + op.n_new]
            if op.add is not None:
                add, n = self._read(op.add, chunk)
                assert 0 <= op.add_off and op.add_off + op.n_new <= n, op
                new = new + add[:, :, op.add_off : op.add_off + op.n_new]
            parts.append(new)
        total = op.n_carry + op.n_new
        kind, key = op.dst.split(":", 1)
        if kind == "emit":
            emitted[key] = torch.cat(parts, dim=2).clone()
            return
        assert total <= self.bufs[key][0].shape[2], (op, "past the plan's capacity")
        if total:
            other = self.bufs[key][1 - self.cur[key]]
            other.fill_(NAN)
            other[:, :, :total] = torch.cat(parts, dim=2)
            self.cur[key] = 1 - self.cur[key]
        self.length[key] = total
        self.longest[key] = max(self.longest[key], total)

    # ---- layers -----------------------------------------------------------------------------------------------------------------------
    def _layer(self, name, x):
        sd, p = self.sd, self.gen.p
        nl = lambda t: F.leaky_relu(t, 0.01)
        nd = self.nodes[name]
        if name == "pqmf.analysis":
            return O.pqmf_analysis(x, sd["pqmf.analysis_weights"], bands=p)
        if name == "pqmf.synthesis":
            return O.pqmf_synthesis(x, sd["pqmf.synthesis_weights"]).sum(1, keepdim=True)
        if name in ("first_conv", "last_conv"):
            return O._conv_reflect(x, sd[name + ".weight"])
        if nd.kind == "unit":
            if name.startswith("encoder_blocks.") and name.endswith(".residuals.0"):
                x = nl(x)
            return O._residual_unit(sd, name, x, nd.dilation)
        if nd.kind == "convT":
            return nl(F.conv_transpose1d(x, O._wn(sd, name), None, stride=nd.stride, padding=nd.stride // 2))
        if name == "latent_conv.1":
            return nl(O._conv_reflect(nl(x), O._wn(sd, name)))
        if name == "latent_conv.3":
            return nl(O._conv_reflect(x, O._wn(sd, name)))
        s = nd.stride   # the encoder blocks' strided convs
        return O._conv_reflect(x, O._wn(sd, name), stride=s, pad=(s - 1, s - 1))

    def _launch(self, op):
        if op.node == "lift":
            h, fb = self.out["last_conv"], self.bufs["lift.operand"][self.cur["lift.operand"]][:, :, : self.length["lift.operand"]]
            assert h.shape[2] == fb.shape[2] == op.l_in
            m = self.gen.pqmf.decimation
            y = torch.tanh(h + torch.cat((fb, torch.zeros(self.rows, m - fb.shape[1], op.l_in, dtype=fb.dtype)), dim=1))
        else:
            assert self.length[op.node] == op.l_in, op
            y = self._layer(op.node, self.bufs[op.node][self.cur[op.node]][:, :, : op.l_in].clone())
        assert y.shape[2] == op.l_out and 0 <= op.lo < op.hi <= op.l_out, (op, y.shape)
        y = y.clone()
        y[:, :, : op.lo] = NAN
        y[:, :, op.hi :] = NAN
        self.out[op.node] = y

    # ---- the driver -------------------------------------------------------------------------------------------------------------------
    def run(self, chunk, final=False):
        """(enhanced, bands) newly final after this push; ``chunk`` (rows, 1, n) float64, n == 0 allowed at the end."""
        ops = self.schedule.push(chunk.shape[2], final)
        emitted = {}
        for op in ops:
            if isinstance(op, streaming.Splice):
                self._splice(op, chunk, emitted)
            else:
                self._launch(op)
        m = self.gen.pqmf.decimation
        return (emitted.get("enhanced", torch.zeros(self.rows, 1, 0, dtype=torch.float64)),
                emitted.get("bands", torch.zeros(self.rows, m, 0, dtype=torch.float64)))


def stream_clip(gen, sd, clip, chunk_samples):
    """The whole ``clip`` (rows, 1, T) through an ``OracleStream`` in pushes of ``chunk_samples`` and a final shorter one.  Returns
    (the list of (enhanced, bands) per call, the stream)."""
    st = OracleStream(gen, sd, chunk_samples, rows=clip.shape[0])
    t, pos, outs = clip.shape[2], 0, []
    while t - pos >= chunk_samples:
        outs.append(st.run(clip[:, :, pos : pos + chunk_samples]))
        pos += chunk_samples
    outs.append(st.run(clip[:, :, pos:], final=True))
    return outs, st
