"""Records the entry lists ``streaming.PoolBook`` makes for the scenario of ``tests/pool_oracle.py`` (chunk 256, 4 slots, the formula
generator with 2 bands): every ``tick`` and ``close``, field by field, as ``tests/golden/pool_entries_256.json``.

    python -m tests.golden.make_pool_entries_golden

The committed file was written by the commit BEFORE ``PoolBook`` knew ``input_rates``: it is what a pool without rated sessions has to
go on making (tests/test_pool_rate_plan.py).  This script uses nothing younger than that commit, so that it can be run there again.
A session is recorded as its slot, a list of stream operations as the SHA-256 of its ``repr``."""
import dataclasses
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)   # formula.py, for tests/ragged_oracle.py

from tests import pool_oracle as P  # noqa: E402
from tests import ragged_oracle as R  # noqa: E402
from vibravox_amd import streaming  # noqa: E402

PATH = os.path.join(HERE, "pool_entries_256.json")


def plain(entry):
    d = {}
    for f in dataclasses.fields(entry):
        v = getattr(entry, f.name)
        if isinstance(v, streaming.Session):
            v = v.slot
        elif f.name == "order":
            v = [s.slot for s in v]
        elif f.name == "ops":
            v = hashlib.sha256(repr(tuple(v)).encode()).hexdigest()
        elif isinstance(v, tuple):
            v = list(v)
        d[f.name] = v
    return [type(entry).__name__, d]


def record(book, open_session=None):
    """Every list ``book`` makes while the scenario runs on it, in order; ``open_session`` opens a session (default ``book.open``)."""
    spec = P.scenario(P.SCENARIO_256)
    out = []

    class Recorder:
        def open(self):
            return (open_session or book.open)()

        def step(self, chunks):
            out.append([plain(e) for e in book.tick(chunks)])
            return {s: None for s in chunks}

        def close(self, session, tail):
            out.append([plain(e) for e in book.close(session, tail.shape[2])])

    P.run_scenario(Recorder(), {name: torch.zeros(1, 1, total) for name, total, _, _ in spec}, 256, spec)
    return out


if __name__ == "__main__":
    gen, _ = R.formula_generator(2, 32)
    lists = record(streaming.PoolBook(gen, 256, 4))
    with open(PATH, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(entries) for entries in lists) + "\n]\n")
    print(f"{PATH}: {len(lists)} lists, {sum(len(e) for e in lists)} entries")
