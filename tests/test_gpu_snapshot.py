"""GPU: ``eben_pack_tensors`` / ``eben_unpack_tensors`` (csrc/snapshot.hip) against bytes assembled on the host.

The oracle is numpy: an image of zeros with every tensor's bytes put at its offset, and ``~np.isfinite`` counts.  Every comparison is
exact.  Tables of 1, 47, 48, 49 and 97 entries (the launch takes 48 a chunk); with B the block's bytes (``eben_pack_plan``) entries of
0, 1, 3, 4, 15, 16, 17, B-4, B, B+4 and 3B+20 bytes, each at sources 0, 4 and 1 bytes off the 16-byte grid (views into one buffer; the
1-byte case is ``uint8``); float32 contents are random bit patterns (1 in 256 has an all-ones exponent) with NaNs of distinct payloads,
both infinities, -0.0 and denormals planted in front."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FILL = 0xA5
EINVAL = -1
SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff], dtype=np.uint32)
GUARD = 48   # bytes of 0xA5 in front of and behind every view (a multiple of 16: the views' alignment is what the case says)


def block_bytes():
    from vibravox_amd import _lib

    b = _lib.pack_block_bytes()
    assert b > 0 and b % 16 == 0
    return b


def sizes():
    b = block_bytes()
    return [0, 1, 3, 4, 15, 16, 17, b - 4, b, b + 4, 3 * b + 20]


@functools.lru_cache(maxsize=None)
def case(n, first_offset=0):
    """n entries: (specs, host bytes of the source buffer, expected image, expected counts, image_bytes).  A spec is (position of the view
    in the buffer, nbytes, kind, image offset); entry k takes size k mod 11 and alignment (k div 11) mod 3, a single entry the largest."""
    rng = np.random.default_rng(1000 + n)
    all_sizes, specs, at, off = sizes(), [], GUARD, first_offset
    for k in range(n):
        j = k + (10 if n == 1 else 0)
        nbytes, align = all_sizes[j % 11], (0, 4, 1)[(j // 11) % 3]
        kind = int(nbytes % 4 == 0 and align != 1)
        pos = (at + 15) // 16 * 16 + align
        specs.append((pos, nbytes, kind, off))
        at = pos + nbytes + GUARD
        off = (off + nbytes + 15) // 16 * 16
    image_bytes = off + 32   # padding behind the last entry too
    src = np.full(at + 16, FILL, dtype=np.uint8)
    image = np.zeros(image_bytes, dtype=np.uint8)
    counts = np.zeros(n, dtype=np.int64)
    for k, (pos, nbytes, kind, o) in enumerate(specs):
        if kind:
            words = rng.integers(0, 1 << 32, size=nbytes // 4, dtype=np.uint64).astype(np.uint32)
            words[:min(len(SPECIALS), words.size)] = SPECIALS[:words.size]
            data = words.view(np.uint8)
            counts[k] = int((~np.isfinite(words.view(np.float32))).sum())
        else:
            data = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
        src[pos:pos + nbytes] = data
        image[o:o + nbytes] = data
    return tuple(specs), src, image, counts, image_bytes


def table_of(specs, base_ptr, order=None):
    from vibravox_amd._lib import EbenPackEntry

    order = list(range(len(specs))) if order is None else order
    table = (EbenPackEntry * len(specs))()
    for slot, k in enumerate(order):
        pos, nbytes, kind, off = specs[k]
        table[slot] = EbenPackEntry(base_ptr + pos, off, nbytes, kind, 0)
    return table


def filled(nbytes):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("n,first_offset", [(1, 0), (1, 32), (47, 0), (48, 0), (49, 0), (97, 0)])
def test_pack_equals_the_host_assembled_image_and_counts(hip, n, first_offset):
    from vibravox_amd._lib import stream

    specs, src_np, want, counts, image_bytes = case(n, first_offset)
    src = torch.from_numpy(src_np).to(DEV)
    assert src.data_ptr() % 16 == 0
    image = filled(image_bytes + GUARD)          # a guard band behind the image
    nonfinite = torch.full((n + 4,), 77, dtype=torch.int32, device=DEV)
    rc = hip.eben_pack_tensors(table_of(specs, src.data_ptr()), n, image.data_ptr(), image_bytes, nonfinite.data_ptr(), stream())
    assert rc == 0, hip.eben_last_error()
    torch.cuda.synchronize()
    got = image.cpu().numpy()
    assert np.array_equal(got[:image_bytes], want)                       # the tensors' bytes and zeros in every padding byte
    assert (got[image_bytes:] == FILL).all()
    assert nonfinite[:n].cpu().tolist() == counts.tolist() and nonfinite[n:].cpu().tolist() == [77] * 4
    assert counts.sum() > 0 or n == 1
    assert torch.equal(src.cpu(), torch.from_numpy(src_np))              # the sources are only read


@pytest.mark.parametrize("n", [1, 47, 48, 49, 97])
def test_unpack_in_shuffled_order_returns_every_tensor_and_nothing_else(hip, n):
    from vibravox_amd._lib import stream

    specs, src_np, image_np, _, image_bytes = case(n)
    image = torch.from_numpy(image_np).to(DEV)
    dst = filled(src_np.size)
    order = np.random.default_rng(n).permutation(n).tolist()
    rc = hip.eben_unpack_tensors(table_of(specs, dst.data_ptr(), order), n, image.data_ptr(), image_bytes, stream())
    assert rc == 0, hip.eben_last_error()
    torch.cuda.synchronize()
    # the source buffer is 0xA5 outside its views: equality is every tensor bit for bit and every guard byte untouched
    assert np.array_equal(dst.cpu().numpy(), src_np)
    assert np.array_equal(image.cpu().numpy(), image_np)


def test_plan_counts_the_blocks(hip):
    from vibravox_amd._lib import EbenPackEntry

    b = block_bytes()
    specs = case(49)[0]
    table = table_of(specs, 4096)
    blocks, size = ctypes.c_int64(-1), ctypes.c_int(-1)
    assert hip.eben_pack_plan(table, 49, ctypes.byref(blocks), ctypes.byref(size)) == 0
    spans = [(specs[k + 1][3] if k + 1 < 49 else (specs[k][3] + specs[k][1] + 15) // 16 * 16) - specs[k][3] for k in range(49)]
    assert size.value == b and blocks.value == sum(-(-s // b) for s in spans)
    assert hip.eben_pack_plan(None, 0, ctypes.byref(blocks), None) == 0 and blocks.value == 0
    assert ctypes.sizeof(EbenPackEntry) == 32


MALFORMED = {
    "a misaligned offset": lambda e, nxt: setattr(e, "image_offset", e.image_offset + 8),
    "an overlap": lambda e, nxt: setattr(e, "nbytes", nxt.image_offset - e.image_offset + 16),
    "an entry out of bounds": lambda e, nxt: setattr(e, "image_offset", 1 << 40),
    "a float32 entry of 4k + 2 bytes": lambda e, nxt: setattr(e, "nbytes", e.nbytes - 2),
}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_a_malformed_table_is_refused_before_any_launch(hip, what):
    from vibravox_amd._lib import stream

    n, bad = 60, 53                              # the bad entry sits in the second chunk: the first one must not have been launched
    specs, src_np, _, _, image_bytes = case(n)
    assert specs[bad][2] == 1 and specs[bad][1] > 16
    src = torch.from_numpy(src_np).to(DEV)
    image, nonfinite = filled(image_bytes), torch.full((n,), 77, dtype=torch.int32, device=DEV)
    table = table_of(specs, src.data_ptr())
    MALFORMED[what](table[bad], table[bad + 1])
    assert hip.eben_pack_tensors(table, n, image.data_ptr(), image_bytes, nonfinite.data_ptr(), stream()) == EINVAL
    assert hip.eben_last_error()
    dst = filled(src_np.size)
    table = table_of(specs, dst.data_ptr())
    MALFORMED[what](table[bad], table[bad + 1])
    assert hip.eben_unpack_tensors(table, n, image.data_ptr(), image_bytes, stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((image == FILL).all()) and bool((dst == FILL).all()) and nonfinite.cpu().tolist() == [77] * n


def test_null_pointers_and_descending_offsets_are_refused(hip):
    from vibravox_amd._lib import stream

    specs, src_np, _, _, image_bytes = case(47)
    src, image = torch.from_numpy(src_np).to(DEV), filled(image_bytes)
    nonfinite = torch.zeros(47, dtype=torch.int32, device=DEV)
    table = table_of(specs, src.data_ptr())
    table[5].tensor = None
    assert hip.eben_pack_tensors(table, 47, image.data_ptr(), image_bytes, nonfinite.data_ptr(), stream()) == EINVAL
    table = table_of(specs, src.data_ptr(), list(reversed(range(47))))   # legal for unpack, not for pack
    assert hip.eben_pack_tensors(table, 47, image.data_ptr(), image_bytes, nonfinite.data_ptr(), stream()) == EINVAL
    table = table_of(specs, src.data_ptr())
    assert hip.eben_pack_tensors(table, 47, None, image_bytes, nonfinite.data_ptr(), stream()) == EINVAL
    assert hip.eben_pack_tensors(table, 47, image.data_ptr(), image_bytes, None, stream()) == EINVAL   # float32 entries need the counters
    assert hip.eben_pack_tensors(table, 0, image.data_ptr(), image_bytes, nonfinite.data_ptr(), stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((image == FILL).all())


def test_snapshot_of_device_tensors_equals_the_host_assembly(hip):
    """The Python face: ``Snapshot.take`` over device tensors (a strided one, an empty one, an int64 one and a 0-dim view among them)
    leaves in pinned memory what ``assemble_host`` builds from the same tensors on the CPU, counters included, twice in a row."""
    from collections import OrderedDict

    from vibravox_amd import checkpoint as C

    g = torch.Generator().manual_seed(4)
    b = block_bytes()
    host = OrderedDict([
        ("a", torch.randn(3 * b // 4 + 5, generator=g)), ("strided", torch.randn(6, 10, generator=g).t()), ("empty", torch.zeros(0, 3)),
        ("steps", torch.arange(7, dtype=torch.int64)), ("bad", torch.tensor([1.0, float("nan"), float("-inf"), -0.0])),
        ("vector", torch.randn(3, generator=g))])
    dev = OrderedDict((k, v.to(DEV)) for k, v in host.items())
    dev["scalar"], host["scalar"] = dev["vector"][1], host["vector"][1]      # 4 bytes off the 16-byte grid
    plan = C.plan_image(host)
    want = C.assemble_host(plan, list(host.values()), torch.empty(plan.image_bytes, dtype=torch.uint8))
    snap = C.Snapshot()

    class State:
        tensors = dev
    for _ in range(3):   # both pinned images, and the first one again
        taken = snap.take(State).wait()
        assert taken.image.is_pinned() and torch.equal(taken.image, want)
        assert taken.nonfinite() == [("bad", 2)]
        assert torch.equal(taken.tensor("strided"), host["strided"]) and taken.tensor("empty").shape == (0, 3)
