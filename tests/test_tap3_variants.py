"""CPU (no GPU): which kernel instantiation every launch of the case table runs, asked of the library's own dispatch decision
(eben_conv1d_variant / eben_bl_conv1d_bwd_dw_variant: the helper tap3_launch and the bl_dw entry points dispatch on), and that the
table reaches every tap3_kernel and bl_dw instantiation the dispatch can pick.  tests/test_gpu_tap3_variants.py runs each case
against a float64 conv; a retuned launch plan that moves a case off its instantiation fails here by name.

tap3_kernel<FM, XRB, IM, NPW, NPX, BL> (tapconv3.hip, launch3_cfg): FM 32-row fragments per block (make_plan3: the rows per group,
shrunk while fewer than 256 blocks of (column tile, batch, phase, group) would run), XRB input-tile staging rows (2 while the
channels fit one tile, else the first of 2 / 3 / 5 whose tile of `XRB * 256 / span` bundles holds a 16-channel chunk: long spans --
stride 4, 41 taps -- need 5), and seven operand forms: plain, mask on load (IM, autograd's input gradient), hi + lo activation
(EBEN_MATH_BF16X2 forward), bf16x3 / bf16x6 pieces, bundle layout with one or two pieces.

Every one of the 84 instantiations is reachable with the default settings, so UNREACHABLE is empty.  In particular the
EBEN_MATH_BF16X6 operand (NPW = 3), sized on the 150 KB split budget, still needs channel chunks with 3- and 5-row staging once a
group's reduction outgrows it (1024 -> 768 channels at 3 taps: the fm*_xrb5_x6 cases).
"""
import ctypes
import itertools
import os

import pytest

from vibravox_amd import ops

BF16, BF16X2, BF16X3, BF16X6 = ops.MATH_BF16, ops.MATH_BF16X2, ops.MATH_BF16X3, ops.MATH_BF16X6
PLAIN, BL = 0, 0x100   # EBEN_LAYOUT_BL
FWD, DX = 0, 1
TAP3, THIN_BL, TAP4 = 1, 2, 3   # EBEN_VARIANT_*


class C:
    """One launch: ConvSpec kwargs (the activations are the GPU test's), batch, length, math, layout, direction (FWD: the layer's
    forward; DX: its input gradient), mask on load, expected (FM, XRB, IM, NPW, NPX, BL) of tap3_kernel, and the knobs (environment)
    the case needs -- none here: every instantiation is reached by a default plan."""

    def __init__(self, kw, batch, length, math, layout, direction, mask_on_load, expect, env=None):
        self.kw, self.batch, self.length, self.math, self.layout = kw, batch, length, math, layout
        self.direction, self.mask_on_load, self.expect, self.env = direction, mask_on_load, tuple(expect), env or {}

    def spec(self):
        return ops.ConvSpec(**self.kw)

    def desc(self, spec=None):
        return ops.conv_desc(spec or self.spec(), self.batch, self.length, self.math | self.layout)


# generated from the plans, then kept: lengths off the 128-column tile and off the stride, B = 1 and single-tile launches,
# odd channel counts per group (3 rows per group: c_out 9 at 3 groups), FM = 4 through column tiles x batch x stride phases
CASES = {
    "fm1_xrb2_plain": C(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16, PLAIN, FWD, 0, (1, 2, 0, 1, 1, 0)),
    "fm1_xrb2_bl": C(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16, BL, FWD, 0, (1, 2, 0, 1, 1, 1)),
    "fm1_xrb2_x2": C(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16X2, PLAIN, FWD, 0, (1, 2, 0, 1, 2, 0)),
    "fm1_xrb2_x3": C(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16X3, PLAIN, FWD, 0, (1, 2, 0, 2, 2, 0)),
    "fm1_xrb2_x3bl": C(dict(c_in=8, c_out=8, ksize=5, stride=4, pad_l=2, pad_r=2), 1, 97, BF16X3, BL, FWD, 0, (1, 2, 0, 2, 2, 1)),
    "fm1_xrb2_x6": C(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16X6, PLAIN, FWD, 0, (1, 2, 0, 3, 3, 0)),
    "fm1_xrb2_im": C(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16, PLAIN, DX, 1, (1, 2, 1, 1, 1, 0)),
    "fm1_xrb3_plain": C(dict(c_in=8, c_out=192, ksize=5, pad_l=2, pad_r=2), 1, 97, BF16, PLAIN, DX, 0, (1, 3, 0, 1, 1, 0)),
    "fm1_xrb3_bl": C(dict(c_in=8, c_out=192, ksize=5, pad_l=2, pad_r=2), 1, 97, BF16, BL, DX, 0, (1, 3, 0, 1, 1, 1)),
    "fm1_xrb3_x2": C(dict(c_in=48, c_out=8, ksize=7, stride=2, pad_l=3, pad_r=3), 1, 97, BF16X2, PLAIN, FWD, 0, (1, 3, 0, 1, 2, 0)),
    "fm1_xrb3_x3": C(dict(c_in=64, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16X3, PLAIN, FWD, 0, (1, 3, 0, 2, 2, 0)),
    "fm1_xrb3_x3bl": C(dict(c_in=64, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16X3, BL, FWD, 0, (1, 3, 0, 2, 2, 1)),
    "fm1_xrb3_x6": C(dict(c_in=96, c_out=8, ksize=7, stride=2, pad_l=3, pad_r=3), 1, 97, BF16X6, PLAIN, FWD, 0, (1, 3, 0, 3, 3, 0)),
    "fm1_xrb3_im": C(dict(c_in=8, c_out=192, ksize=5, pad_l=2, pad_r=2), 1, 97, BF16, PLAIN, DX, 1, (1, 3, 1, 1, 1, 0)),
    "fm1_xrb5_plain": C(dict(c_in=48, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, BF16, PLAIN, FWD, 0, (1, 5, 0, 1, 1, 0)),
    "fm1_xrb5_bl": C(dict(c_in=48, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, BF16, BL, FWD, 0, (1, 5, 0, 1, 1, 1)),
    "fm1_xrb5_x2": C(dict(c_in=24, c_out=9, ksize=15, stride=4, groups=3, pad_l=7, pad_r=7), 1, 97, BF16X2, PLAIN, FWD, 0, (1, 5, 0, 1, 2, 0)),
    "fm1_xrb5_x3": C(dict(c_in=24, c_out=9, ksize=15, stride=4, groups=3, pad_l=7, pad_r=7), 1, 97, BF16X3, PLAIN, FWD, 0, (1, 5, 0, 2, 2, 0)),
    "fm1_xrb5_x3bl": C(dict(c_in=24, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, BF16X3, BL, FWD, 0, (1, 5, 0, 2, 2, 1)),
    "fm1_xrb5_x6": C(dict(c_in=48, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, BF16X6, PLAIN, FWD, 0, (1, 5, 0, 3, 3, 0)),
    "fm1_xrb5_im": C(dict(c_in=8, c_out=192, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, BF16, PLAIN, DX, 1, (1, 5, 1, 1, 1, 0)),
    "fm2_xrb2_plain": C(dict(c_in=512, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 0, (2, 2, 0, 1, 1, 0)),
    "fm2_xrb2_bl": C(dict(c_in=512, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, BL, DX, 0, (2, 2, 0, 1, 1, 1)),
    "fm2_xrb2_x2": C(dict(c_in=24, c_out=36, ksize=1, groups=3), 8, 4099, BF16X2, PLAIN, FWD, 0, (2, 2, 0, 1, 2, 0)),
    "fm2_xrb2_x3": C(dict(c_in=512, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X3, PLAIN, DX, 0, (2, 2, 0, 2, 2, 0)),
    "fm2_xrb2_x3bl": C(dict(c_in=32, c_out=1024, ksize=5, stride=4, groups=4, pad_l=2, pad_r=2), 16, 97, BF16X3, BL, FWD, 0, (2, 2, 0, 2, 2, 1)),
    "fm2_xrb2_x6": C(dict(c_in=512, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X6, PLAIN, DX, 0, (2, 2, 0, 3, 3, 0)),
    "fm2_xrb2_im": C(dict(c_in=512, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 1, (2, 2, 1, 1, 1, 0)),
    "fm2_xrb3_plain": C(dict(c_in=48, c_out=128, ksize=5, groups=4, pad_l=2, pad_r=2), 8, 4099, BF16, PLAIN, DX, 0, (2, 3, 0, 1, 1, 0)),
    "fm2_xrb3_bl": C(dict(c_in=48, c_out=128, ksize=5, groups=4, pad_l=2, pad_r=2), 8, 4099, BF16, BL, DX, 0, (2, 3, 0, 1, 1, 1)),
    "fm2_xrb3_x2": C(dict(c_in=32, c_out=128, ksize=7, stride=2, groups=4, pad_l=3, pad_r=3), 8, 4099, BF16X2, PLAIN, FWD, 0, (2, 3, 0, 1, 2, 0)),
    "fm2_xrb3_x3": C(dict(c_in=36, c_out=96, ksize=3, stride=2, groups=3, pad_l=1, pad_r=1), 8, 4099, BF16X3, PLAIN, DX, 0, (2, 3, 0, 2, 2, 0)),
    "fm2_xrb3_x3bl": C(dict(c_in=192, c_out=1024, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 16, 97, BF16X3, BL, FWD, 0, (2, 3, 0, 2, 2, 1)),
    "fm2_xrb3_x6": C(dict(c_in=512, c_out=768, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X6, PLAIN, DX, 0, (2, 3, 0, 3, 3, 0)),
    "fm2_xrb3_im": C(dict(c_in=48, c_out=128, ksize=5, groups=4, pad_l=2, pad_r=2), 8, 4099, BF16, PLAIN, DX, 1, (2, 3, 1, 1, 1, 0)),
    "fm2_xrb5_plain": C(dict(c_in=48, c_out=128, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 4099, BF16, PLAIN, DX, 0, (2, 5, 0, 1, 1, 0)),
    "fm2_xrb5_bl": C(dict(c_in=48, c_out=128, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 4099, BF16, BL, DX, 0, (2, 5, 0, 1, 1, 1)),
    "fm2_xrb5_x2": C(dict(c_in=768, c_out=1024, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16X2, PLAIN, FWD, 0, (2, 5, 0, 1, 2, 0)),
    "fm2_xrb5_x3": C(dict(c_in=384, c_out=1024, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 701, BF16X3, PLAIN, FWD, 0, (2, 5, 0, 2, 2, 0)),
    "fm2_xrb5_x3bl": C(dict(c_in=384, c_out=1024, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 701, BF16X3, BL, FWD, 0, (2, 5, 0, 2, 2, 1)),
    "fm2_xrb5_x6": C(dict(c_in=1024, c_out=768, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 97, BF16X6, PLAIN, DX, 0, (2, 5, 0, 3, 3, 0)),
    "fm2_xrb5_im": C(dict(c_in=48, c_out=128, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 4099, BF16, PLAIN, DX, 1, (2, 5, 1, 1, 1, 0)),
    "fm3_xrb2_plain": C(dict(c_in=768, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 0, (3, 2, 0, 1, 1, 0)),
    "fm3_xrb2_bl": C(dict(c_in=768, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, BL, DX, 0, (3, 2, 0, 1, 1, 1)),
    "fm3_xrb2_x2": C(dict(c_in=24, c_out=72, ksize=1, groups=3), 8, 4099, BF16X2, PLAIN, FWD, 0, (3, 2, 0, 1, 2, 0)),
    "fm3_xrb2_x3": C(dict(c_in=768, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X3, PLAIN, DX, 0, (3, 2, 0, 2, 2, 0)),
    "fm3_xrb2_x3bl": C(dict(c_in=24, c_out=72, ksize=1, groups=3), 8, 4099, BF16X3, BL, FWD, 0, (3, 2, 0, 2, 2, 1)),
    "fm3_xrb2_x6": C(dict(c_in=768, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X6, PLAIN, DX, 0, (3, 2, 0, 3, 3, 0)),
    "fm3_xrb2_im": C(dict(c_in=768, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 1, (3, 2, 1, 1, 1, 0)),
    "fm3_xrb3_plain": C(dict(c_in=768, c_out=384, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 0, (3, 3, 0, 1, 1, 0)),
    "fm3_xrb3_bl": C(dict(c_in=768, c_out=384, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, BL, DX, 0, (3, 3, 0, 1, 1, 1)),
    "fm3_xrb3_x2": C(dict(c_in=192, c_out=768, ksize=1, groups=4), 1, 4099, BF16X2, PLAIN, FWD, 0, (3, 3, 0, 1, 2, 0)),
    "fm3_xrb3_x3": C(dict(c_in=768, c_out=384, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X3, PLAIN, DX, 0, (3, 3, 0, 2, 2, 0)),
    "fm3_xrb3_x3bl": C(dict(c_in=192, c_out=768, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 16, 301, BF16X3, BL, FWD, 0, (3, 3, 0, 2, 2, 1)),
    "fm3_xrb3_x6": C(dict(c_in=768, c_out=768, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X6, PLAIN, DX, 0, (3, 3, 0, 3, 3, 0)),
    "fm3_xrb3_im": C(dict(c_in=768, c_out=384, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 1, (3, 3, 1, 1, 1, 0)),
    "fm3_xrb5_plain": C(dict(c_in=768, c_out=512, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16, PLAIN, DX, 0, (3, 5, 0, 1, 1, 0)),
    "fm3_xrb5_bl": C(dict(c_in=768, c_out=512, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16, BL, DX, 0, (3, 5, 0, 1, 1, 1)),
    "fm3_xrb5_x2": C(dict(c_in=1024, c_out=768, ksize=1, groups=4), 1, 4099, BF16X2, PLAIN, FWD, 0, (3, 5, 0, 1, 2, 0)),
    "fm3_xrb5_x3": C(dict(c_in=192, c_out=576, ksize=15, stride=4, groups=3, pad_l=7, pad_r=7), 5, 4099, BF16X3, PLAIN, FWD, 0, (3, 5, 0, 2, 2, 0)),
    "fm3_xrb5_x3bl": C(dict(c_in=256, c_out=384, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 4099, BF16X3, BL, FWD, 0, (3, 5, 0, 2, 2, 1)),
    "fm3_xrb5_x6": C(dict(c_in=768, c_out=768, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16X6, PLAIN, DX, 0, (3, 5, 0, 3, 3, 0)),
    "fm3_xrb5_im": C(dict(c_in=768, c_out=512, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16, PLAIN, DX, 1, (3, 5, 1, 1, 1, 0)),
    "fm4_xrb2_plain": C(dict(c_in=1024, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 0, (4, 2, 0, 1, 1, 0)),
    "fm4_xrb2_bl": C(dict(c_in=1024, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, BL, DX, 0, (4, 2, 0, 1, 1, 1)),
    "fm4_xrb2_x2": C(dict(c_in=32, c_out=128, ksize=1, groups=4), 8, 4099, BF16X2, PLAIN, FWD, 0, (4, 2, 0, 1, 2, 0)),
    "fm4_xrb2_x3": C(dict(c_in=1024, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X3, PLAIN, DX, 0, (4, 2, 0, 2, 2, 0)),
    "fm4_xrb2_x3bl": C(dict(c_in=24, c_out=1152, ksize=3, stride=2, groups=3, pad_l=1, pad_r=1), 16, 301, BF16X3, BL, FWD, 0, (4, 2, 0, 2, 2, 1)),
    "fm4_xrb2_x6": C(dict(c_in=1024, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X6, PLAIN, DX, 0, (4, 2, 0, 3, 3, 0)),
    "fm4_xrb2_im": C(dict(c_in=1024, c_out=32, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 1, (4, 2, 1, 1, 1, 0)),
    "fm4_xrb3_plain": C(dict(c_in=1024, c_out=256, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 0, (4, 3, 0, 1, 1, 0)),
    "fm4_xrb3_bl": C(dict(c_in=1024, c_out=256, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, BL, DX, 0, (4, 3, 0, 1, 1, 1)),
    "fm4_xrb3_x2": C(dict(c_in=24, c_out=768, ksize=3, stride=2, groups=3, pad_l=1, pad_r=1), 5, 2103, BF16X2, PLAIN, FWD, 0, (4, 3, 0, 1, 2, 0)),
    "fm4_xrb3_x3": C(dict(c_in=1024, c_out=256, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16X3, PLAIN, DX, 0, (4, 3, 0, 2, 2, 0)),
    "fm4_xrb3_x3bl": C(dict(c_in=32, c_out=128, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 8191, BF16X3, BL, FWD, 0, (4, 3, 0, 2, 2, 1)),
    "fm4_xrb3_x6": C(dict(c_in=1024, c_out=768, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16X6, PLAIN, DX, 0, (4, 3, 0, 3, 3, 0)),
    "fm4_xrb3_im": C(dict(c_in=1024, c_out=256, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 8, 97, BF16, PLAIN, DX, 1, (4, 3, 1, 1, 1, 0)),
    "fm4_xrb5_plain": C(dict(c_in=1024, c_out=256, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16, PLAIN, DX, 0, (4, 5, 0, 1, 1, 0)),
    "fm4_xrb5_bl": C(dict(c_in=1024, c_out=256, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16, BL, DX, 0, (4, 5, 0, 1, 1, 1)),
    "fm4_xrb5_x2": C(dict(c_in=1024, c_out=1024, ksize=1, groups=4), 1, 4099, BF16X2, PLAIN, FWD, 0, (4, 5, 0, 1, 2, 0)),
    "fm4_xrb5_x3": C(dict(c_in=192, c_out=768, ksize=15, stride=4, groups=3, pad_l=7, pad_r=7), 5, 4099, BF16X3, PLAIN, FWD, 0, (4, 5, 0, 2, 2, 0)),
    "fm4_xrb5_x3bl": C(dict(c_in=192, c_out=768, ksize=15, stride=4, groups=3, pad_l=7, pad_r=7), 5, 4099, BF16X3, BL, FWD, 0, (4, 5, 0, 2, 2, 1)),
    "fm4_xrb5_x6": C(dict(c_in=1024, c_out=768, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16X6, PLAIN, DX, 0, (4, 5, 0, 3, 3, 0)),
    "fm4_xrb5_im": C(dict(c_in=1024, c_out=256, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 8, 301, BF16, PLAIN, DX, 1, (4, 5, 1, 1, 1, 0)),
    # the reference's own discriminator geometries nobody checked numerically: DiscriminatorEBENMultiScales(q=3, min_channels=24) --
    # groups of 3, 8 input channels per group at the first strided layer -- and (q=4, min_channels=48): 12 per group
    "disc_q3_l1_d3_fwd": C(dict(c_in=24, c_out=48, ksize=7, stride=2, dilation=3, groups=3, pad_l=3, pad_r=3), 2, 1001, BF16, PLAIN, FWD, 0, (1, 2, 0, 1, 1, 0)),
    "disc_q3_l1_d3_im": C(dict(c_in=24, c_out=48, ksize=7, stride=2, dilation=3, groups=3, pad_l=3, pad_r=3), 2, 1001, BF16, PLAIN, DX, 1, (1, 2, 1, 1, 1, 0)),
    "disc_q3_l1_bl_fwd": C(dict(c_in=24, c_out=48, ksize=7, stride=2, groups=3, pad_l=3, pad_r=3), 3, 260, BF16, BL, FWD, 0, (1, 2, 0, 1, 1, 1)),
    "disc_q3_l6_d2_dx": C(dict(c_in=768, c_out=768, ksize=5, dilation=2, groups=3, pad_l=2, pad_r=2), 2, 131, BF16, PLAIN, DX, 0, (1, 3, 0, 1, 1, 0)),
    "disc_q4_l1_d2_fwd": C(dict(c_in=48, c_out=96, ksize=7, stride=2, dilation=2, groups=4, pad_l=3, pad_r=3), 2, 1001, BF16, PLAIN, FWD, 0, (1, 2, 0, 1, 1, 0)),
    "disc_q4_l1_d1_dx": C(dict(c_in=48, c_out=96, ksize=7, stride=2, groups=4, pad_l=3, pad_r=3), 3, 260, BF16, PLAIN, DX, 0, (1, 2, 0, 1, 1, 0)),
    "disc_q4_l1_bl_fwd": C(dict(c_in=48, c_out=96, ksize=7, stride=2, dilation=3, groups=4, pad_l=3, pad_r=3), 2, 1001, BF16, BL, FWD, 0, (1, 2, 0, 1, 1, 1)),
    "disc_q4_l6_x3_fwd": C(dict(c_in=1536, c_out=1536, ksize=5, groups=4, pad_l=2, pad_r=2), 2, 131, BF16X3, PLAIN, FWD, 0, (1, 2, 0, 2, 2, 0)),
}

# The bundle-layout input gradient (eben_bl_conv1d_bwd_dx) takes one gradient plane: its launches are EBEN_MATH_BF16, and the
# two-piece bundle-layout forms are reached by forwards.
# instantiations of launch3_cfg no default plan can reach, each with the make_plan3 rule that excludes it: none (see the docstring)
UNREACHABLE = {}

FORMS = [(0, 1, 1, 0), (1, 1, 1, 0), (0, 1, 2, 0), (0, 2, 2, 0), (0, 3, 3, 0), (0, 1, 1, 1), (0, 2, 2, 1)]   # (IM, NPW, NPX, BL)
ALL_TAP3 = {(fm, xrb) + f for fm in (1, 2, 3, 4) for xrb in (2, 3, 5) for f in FORMS}


class D:
    """One bundle-layout weight gradient: ConvSpec kwargs, batch, length, expected (FM, FN, XC, WN, grouped by _multi)."""

    def __init__(self, kw, batch, length, expect):
        self.kw, self.batch, self.length, self.expect = kw, batch, length, tuple(expect)

    def spec(self):
        return ops.ConvSpec(**self.kw)

    def desc(self):
        return ops.conv_desc(self.spec(), self.batch, self.length, BF16 | BL)


DW_CASES = {
    "dw_fm1_fn1": D(dict(c_in=8, c_out=8, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, (1, 1, 0, 2, 1)),
    "dw_fm1_fn2": D(dict(c_in=8, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, (1, 2, 0, 2, 1)),
    "dw_fm1_fn3": D(dict(c_in=24, c_out=8, ksize=7, stride=2, pad_l=3, pad_r=3), 1, 97, (1, 3, 0, 2, 1)),
    "dw_fm1_fn3_xc": D(dict(c_in=24, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, (1, 3, 1, 2, 0)),
    "dw_fm1_fn4": D(dict(c_in=192, c_out=8, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, (1, 4, 0, 2, 1)),
    "dw_fm1_fn4_xc": D(dict(c_in=8, c_out=8, ksize=41, stride=4, pad_l=20, pad_r=20), 1, 97, (1, 4, 1, 2, 0)),
    "dw_fm2_fn1": D(dict(c_in=8, c_out=96, ksize=3, stride=2, pad_l=1, pad_r=1), 1, 97, (2, 1, 0, 2, 1)),
    "dw_fm2_fn2": D(dict(c_in=8, c_out=96, ksize=15, stride=4, pad_l=7, pad_r=7), 1, 97, (2, 2, 0, 2, 1)),
    "dw_fm2_fn3": D(dict(c_in=48, c_out=96, ksize=3, stride=2, groups=4, pad_l=1, pad_r=1), 3, 301, (2, 3, 0, 2, 1)),
    "dw_fm2_fn3_xc": D(dict(c_in=24, c_out=96, ksize=15, stride=4, pad_l=7, pad_r=7), 2, 701, (2, 3, 1, 2, 0)),
    "dw_fm2_fn3_xc_wide": D(dict(c_in=48, c_out=96, ksize=15, stride=4, groups=4, pad_l=7, pad_r=7), 1, 97, (2, 3, 1, 4, 0)),
    "dw_fm2_fn4": D(dict(c_in=192, c_out=96, ksize=11, pad_l=5, pad_r=5), 1, 97, (2, 4, 0, 2, 1)),
    "dw_fm2_fn4_xc": D(dict(c_in=8, c_out=96, ksize=41, stride=4, pad_l=20, pad_r=20), 3, 1001, (2, 4, 1, 2, 0)),
    # the discriminator at (q=3, min_channels=24): 8 -> 16 channels per group at the first strided layer
    "dw_disc_q3_l1": D(dict(c_in=24, c_out=48, ksize=7, stride=2, dilation=2, groups=3, pad_l=3, pad_r=3), 2, 1001, (1, 1, 0, 2, 1)),
}
DW_UNREACHABLE = {}
ALL_BLDW = {(fm, fn, 0, 2) for fm in (1, 2) for fn in (1, 2, 3, 4)} | {(fm, fn, 1, 2) for fm in (1, 2) for fn in (3, 4)} | {(2, 3, 1, 4)}
ALL_BLDW_MULTI = {(fm, fn) for fm in (1, 2) for fn in (1, 2, 3, 4)}


@pytest.fixture(scope="module")
def lib():
    from vibravox_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def variant(lib, case, which=None, mask_on_load=None):
    out = (ctypes.c_int * 8)()
    d = case.desc()
    rc = lib.eben_conv1d_variant(ctypes.byref(d), case.direction if which is None else which,
                                 case.mask_on_load if mask_on_load is None else mask_on_load, out, 8)
    return rc, tuple(out)


def dw_variant(lib, case):
    out = (ctypes.c_int * 5)()
    d = case.desc()
    rc = lib.eben_bl_conv1d_bwd_dw_variant(ctypes.byref(d), out, 5)
    return rc, tuple(out)


def tap3_tuple(lib, case):
    rc, v = variant(lib, case)
    assert rc == 0, lib.eben_last_error()
    return v


@pytest.mark.parametrize("name", list(CASES))
def test_case_runs_its_tap3_instantiation(lib, name):
    case = CASES[name]
    gen, fm, xrb, im, npw, npx, bl, kernel = tap3_tuple(lib, case)
    assert (gen, kernel) == (ops.CONV_ROUTE_TAP3, TAP3), (name, gen, kernel)
    assert (fm, xrb, im, npw, npx, bl) == case.expect, (name, (fm, xrb, im, npw, npx, bl))
    # the bundle-layout input gradient takes one gradient plane: two-piece bundle-layout cases are forwards
    assert not (case.layout == BL and case.math == BF16X3 and case.direction == DX), name


def test_table_reaches_every_tap3_instantiation(lib):
    reached = {tap3_tuple(lib, c)[1:7] for c in CASES.values()}
    assert not set(UNREACHABLE) & reached, set(UNREACHABLE) & reached
    assert reached | set(UNREACHABLE) == ALL_TAP3, sorted(ALL_TAP3 - reached - set(UNREACHABLE))
    assert all(reason for reason in UNREACHABLE.values())


@pytest.mark.parametrize("name", list(DW_CASES))
def test_weight_gradient_case_runs_its_bl_dw_instantiation(lib, name):
    rc, v = dw_variant(lib, DW_CASES[name])
    assert rc == 0, lib.eben_last_error()
    assert v == DW_CASES[name].expect, (name, v)


def test_table_reaches_every_bl_dw_instantiation(lib):
    reached = [dw_variant(lib, c)[1] for c in DW_CASES.values()]
    assert {v[:4] for v in reached} | set(DW_UNREACHABLE) == ALL_BLDW, sorted(ALL_BLDW - {v[:4] for v in reached})
    # bl_dw_multi_kernel<FM, FN>: the problems _multi groups (no contiguous-X rows, not the eight-wave form)
    assert {v[:2] for v in reached if v[4]} == ALL_BLDW_MULTI
    assert all(v[2] == 0 and v[3] == 2 for v in reached if v[4])


def test_variant_query_refuses_what_the_launch_refuses(lib):
    x3 = CASES["fm1_xrb2_x3"]
    assert variant(lib, x3, which=1, mask_on_load=1)[0] == -3          # split operand with a mask on load: no instantiation
    assert variant(lib, CASES["fm1_xrb2_bl"], which=1, mask_on_load=1)[0] == -3   # bundle layout: the mask is the epilogue's
    assert variant(lib, CASES["fm1_xrb2_plain"], which=0, mask_on_load=1)[0] == -1   # forwards never mask on load
    out = (ctypes.c_int * 4)()
    d = x3.desc()
    assert lib.eben_conv1d_variant(ctypes.byref(d), 0, 0, out, 4) == -1
    # a layer outside the bf16 kernels reports its generation and nothing else
    f32 = ops.conv_desc(x3.spec(), 1, 97, ops.MATH_F32)
    full = (ctypes.c_int * 8)()
    assert lib.eben_conv1d_variant(ctypes.byref(f32), 0, 0, full, 8) == 0
    assert full[0] == lib.eben_conv1d_kernel_generation(ctypes.byref(f32), 0) and tuple(full)[1:] == (0,) * 7


def test_variant_query_names_the_other_kernels(lib):
    """The same query reports the thin bundle-layout kernel and the persistent tap4 form where the dispatch sends a launch there."""
    thin = C(dict(c_in=16, c_out=64, ksize=41, stride=4, groups=4, pad_l=20, pad_r=20), 2, 1001, BF16, BL, FWD, 0, ())
    assert tap3_tuple(lib, thin)[7] == THIN_BL
    big = C(dict(c_in=1536, c_out=1536, ksize=5, groups=4, pad_l=2, pad_r=2), 2, 131, BF16, BL, FWD, 0, ())
    v = tap3_tuple(lib, big)
    assert (v[0], v[7]) == (ops.CONV_ROUTE_TAP4, TAP4)
