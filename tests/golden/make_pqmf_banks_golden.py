"""Generate tests/golden/pqmf_banks_golden.npz by running the REFERENCE PseudoQMFBanks / EBENGenerator at bank sizes
other than the (4, 32) of the EBEN configurations.

Runs only in the build container (imports the reference read-only, exactly as ``make_golden.py`` does).  Inputs and
weights are the closed-form tensors of ``formula.py``.

What is frozen (float32 as the reference computes it, unless noted):
  * ``bank{M}x{N}/cutoff`` (float64), ``/analysis``, ``/synthesis`` for (M, N) = (8, 64), (16, 256), (32, 1024), (4, 512)
  * for (32, 1024) on a (2, 1, 7328) clip and (16, 256) on a (3, 1, 2128) clip of ``formula_tensor`` noise:
      ``out{M}x{N}/analysis``            forward(x, "analysis"), in full
      ``out{M}x{N}/synthesis_sum:every3``   sum over bands of forward(analysis, "synthesis"), time samples 0, 3, 6, ...
      ``out{M}x{N}/synthesis:every{S}``     forward(analysis, "synthesis") per band, time samples 0, S, 2 S, ... (S = 97 / 29)
    (the per-band output of the larger bank alone is 1.9 MB in full; the strides are coprime to the decimation, so every
    polyphase component of every band is sampled)
  * EBENGenerator(m=4, n=512, p=2) with ``formula_state_dict`` weights (tag "G512") on ``formula_audio("g512_in", 1, 1536)``:
      ``gen512/enhanced``, ``gen512/bands`` in full, ``gen512/grad_in`` = d (enhanced * s).sum() / d input with
      s = ``formula_audio("g512_seed", 1, 1536, amp=1.0)``, and the same objective's gradients ``gen512/grad_first_conv``,
      ``gen512/grad_last_conv`` w.r.t. ``first_conv.weight`` / ``last_conv.weight``

Usage:  python tests/golden/make_pqmf_banks_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from formula import formula_audio, formula_tensor  # noqa: E402
from make_golden import import_reference, load_formula  # noqa: E402

BANKS = ((8, 64), (16, 256), (32, 1024), (4, 512))
CLIPS = {(32, 1024): ((2, 1, 7328), 97), (16, 256): ((3, 1, 2128), 29)}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = import_reference()
    out = {}
    for m, n in BANKS:
        pq = R["PQMF"](decimation=m, kernel_size=n)
        tag = f"{m}x{n}"
        out[f"bank{tag}/cutoff"] = np.array(pq._cutoff_ratio, dtype=np.float64)
        out[f"bank{tag}/analysis"] = pq.analysis_weights.detach().numpy().copy()
        out[f"bank{tag}/synthesis"] = pq.synthesis_weights.detach().numpy().copy()
        if (m, n) not in CLIPS:
            continue
        shape, every = CLIPS[(m, n)]
        x = formula_tensor(f"pqmf_in/{tag}", shape)
        with torch.no_grad():
            ana = pq(x, "analysis")
            syn = pq(ana, "synthesis")
        assert syn.shape == (shape[0], m, shape[2]), syn.shape
        out[f"out{tag}/analysis"] = ana.numpy().copy()
        out[f"out{tag}/synthesis_sum:every3"] = syn.sum(dim=1, keepdim=True)[..., ::3].numpy().copy()
        out[f"out{tag}/synthesis:every{every}"] = syn[..., ::every].numpy().copy()
        print(tag, "cutoff", pq._cutoff_ratio, "analysis", tuple(ana.shape), "synthesis", tuple(syn.shape))

    gen = R["G"](m=4, n=512, p=2)
    load_formula(gen, "G512")
    x = gen.cut_to_valid_length(formula_audio("g512_in", 1, 1536)).clone().requires_grad_(True)
    assert x.shape[2] == 1536
    enhanced, bands = gen(x)
    seed = formula_audio("g512_seed", 1, enhanced.shape[2], amp=1.0)
    (enhanced * seed).sum().backward()
    out["gen512/enhanced"] = enhanced.detach().numpy().copy()
    out["gen512/bands"] = bands.detach().numpy().copy()
    out["gen512/grad_in"] = x.grad.numpy().copy()
    out["gen512/grad_first_conv"] = gen.first_conv.weight.grad.numpy().copy()
    out["gen512/grad_last_conv"] = gen.last_conv.weight.grad.numpy().copy()
    print("generator n=512: enhanced", tuple(enhanced.shape), "bands", tuple(bands.shape))

    path = os.path.join(HERE, "pqmf_banks_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
