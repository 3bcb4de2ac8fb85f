"""Every instantiation of the stride-1 LDS halo-tile conv, checked element-wise against float64.

``dispatch_ct`` (conv_tile.hip) sends a stride-1 launch - a forward conv, or an input gradient, which is the same kernel
over dy with the transposed, tap-flipped filter - to one ``launch_ct<WM, WN, TM, TN, TPK, MASK, T, WK, SIMPLE>`` of the
translation units conv_tile_{narrow, narrow_masked, n128, n144, wide, masked, small, tm3, simple_narrow, simple_n128,
simple_small, f32, f32_wide, f32_masked}.hip.  ``INSTANTIATION_ROWS`` below has one row (or more) for each of them that a
call can reach, ``UNREACHABLE`` names the others with the check that keeps every call away, and
tests/test_kernel_bounds.py compares the union of the two with the ``launch_ct<...>`` the sources hold.

Every case
* has bf16-exact operands - in the fp32 rows too - with weights scaled by 1 / sqrt(taps * reduction channels);
* reads its input from the channel window [8, 8 + C) of a wider NDHWC buffer whose other channels hold NaN (residuals,
  accumulated tensors and mask sources likewise) and writes a ``kb.Guarded`` buffer with a channel window, compared
  after every launch.  The in-place forms read and write disjoint windows of ONE guarded buffer: the window that is read
  lies outside the output window, so the guard comparison is also the proof that it kept its bits;
* is held to ``kb.ref_fwd`` / ``kb.ref_dgrad`` with ``kb.bound(ref, A, K, rho)``: K = taps * reduction channels, + WK where
  WK > 1 waves share the K-steps, + 1 for an ``act = 2`` or ``acc_src`` join; rho = 2^-8 for bf16 stores, 0 for fp32
  and planar outputs; accumulated values are test operands (exact in bf16), so rho is paid on |ref| only;
* asserts the witness ``hip_ops.last_tile_instantiation()`` - the nine template parameters and a launch count that
  advanced by exactly one, so the call was served by the halo-tile kernel and the record is its own - and the plan
  ``hip_ops.last_tile_plan()`` (tile, NTW, groups, ksplit = 1: the cases pass no workspace, except ``split`` below).

Instantiation rows.  A row names produced channels N and reduction channels R.  Unmasked rows run the forward conv
R -> N with bias + LeakyReLU + alpha + a residual from another tensor, and the input gradient of a conv N -> R with
alpha (dx has N channels): both launches take the same instantiation.  Masked rows run the production form of the
dense-block backward instead: the masked input gradient accumulated in place, dx and dy in two windows of one buffer.
N is never a multiple of 16 (a ragged last n-tile; 144 excepted) and, where the workgroups come in channel groups, the
last group is ragged as well (N 104 on 64-wide groups, 200 on 128-wide ones).  Switches: NS = WSR_CT_NOSMALL=1,
NT = WSR_CT_NO_TM3=1, S0 = WSR_CT_SIMPLE=0, NN = WSR_CT_NO_N128=1, M0 / M1 = WSR_CT_SMALL_MODE.  Volumes
(``pick_tile``, conv_tile_impl.h):

=====  ==============  ====================================================================================================
z17    (9, 17, 17)     Z > 16 and no multiple of 16: z tiles of 8, the third holds one level; 512 voxels -> 8x8x8,
                       384 -> 5x9x8 (the search branch: 48 is no power of two), 256 -> 4x8x8, 128 -> 4x4x8: at least
                       two tiles and a ragged last one along x, y and z for each
z17s   (9, 9, 17)      the same for the 512-voxel tiles only: the 5x5x5 144-wide rows (2.6 MMAC per voxel)
z10    (13, 13, 10)    B = 2; the production level count: one z tile, an x-y budget that is no power of two (51, 38, 25,
                       12): 7x7x10, 5x7x10, 5x5x10, 3x4x10, ragged in x and y
big    (32, 32, 128)   nothing forced: 256 tiles of 4x8x16, more than one round of 384-voxel tiles - the route of the
                       benchmarked volumes (512-voxel SIMPLE forms); reference on the first and last two x planes
mid    (32, 32, 64)    nothing forced: one round either way, so the 384-voxel SIMPLE forms (3x8x16)
=====  ==============  ====================================================================================================

TPK = 1 (32 channels of one tap) needs a 1x1x1 conv that the streaming kernel does not take: the forward rows carry a
``chan_scale``, the input gradients have shapes outside its instantiations (it covers 128 <-> 256 only); the witness
holds both.  The 144-wide TPK = 1 form needs 256 chunks of 32 channels: R = 8192.  TPK = 4 takes R = 24 (bf16) and
R = 12 (fp32), reduction widths without whole tap-pair chunks.

Epilogue rows (``FWD_FORMS`` / ``DGRAD_FORMS`` on the ``CARRIERS``, volume z10): a 32-wide (NTW 2), a 128-wide and a
wide / masked instantiation, bf16 under WSR_CT_SIMPLE = 1 and 0 and fp32; the witness shows SIMPLE = 0 wherever the
SIMPLE form has to decline (``chan_scale``, planar output, an unaligned window, up-sampling, a mask that ends inside a
4-channel group).  The parity and lattice forms (``wsr_conv_t.lat``) stay with the sub-pixel tests of
test_hip_kernels.py.

Mask sign.  Every saved output that feeds a mask carries +0.0, -0.0, the smallest positive and negative subnormals, the
smallest normal and a large negative value at the first voxel, a middle one and the last voxel (of the last ragged
tile), in the first and the last channels of the mask window; the expectation is the reference's ``y > 0``.  NaN in a
saved output is outside the contract.

Declined launches return False, leave a guarded output bit-for-bit untouched and the launch count where it was.
"""
import functools
import math

import pytest
import torch

from conftest import reload_wsr_env
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF, "fp32": F32}
NAN = float("nan")
ALPHA, BETA, SLOPE, MSLOPE, ACC_BETA = 0.7, 0.3, 0.2, 0.2, 0.5
IN_OFF, OUT_OFF = 8, 4

VOLUMES = {"z17": ((9, 17, 17), 1), "z17s": ((9, 9, 17), 1), "z10": ((13, 13, 10), 2), "big": ((32, 32, 128), 1),
           "mid": ((32, 32, 64), 1), "ups": ((7, 6, 10), 2)}
SLABBED = {"big": 2, "mid": 2}  # x planes of the first and of the last x tile that the float64 reference covers
SWITCHES = {"NS": ("WSR_CT_NOSMALL", 1), "NT": ("WSR_CT_NO_TM3", 1), "S0": ("WSR_CT_SIMPLE", 0), "S1": ("WSR_CT_SIMPLE", 1),
            "NN": ("WSR_CT_NO_N128", 1), "M0": ("WSR_CT_SMALL_MODE", 0), "M1": ("WSR_CT_SMALL_MODE", 1)}
K3, K5, K1 = (3, 3, 3), (5, 5, 5), (1, 1, 1)

# id, dtype, N produced, R reduction, kernel, volume, switches, masked,
#   instantiation (WM, WN, TM, TN, TPK, MASK, F32, WK, SIMPLE), plan (TX, TY, TZ, NTW, groups)
INSTANTIATION_ROWS = [
    # ---- bf16, tap pairs (TPK 2), Z > 16 -------------------------------------------------------------------------------
    ("n16_z17", "bf16", 8, 32, K3, "z17", "NS", False, (8, 1, 4, 1, 2, 0, 0, 1, 0), (8, 8, 8, 1, 1)),
    ("n32_z17", "bf16", 24, 32, K3, "z17", "NS NT S0", False, (8, 1, 4, 2, 2, 0, 0, 1, 0), (8, 8, 8, 2, 1)),
    ("n64_z17", "bf16", 40, 32, K3, "z17", "NS", False, (4, 1, 4, 4, 2, 0, 0, 1, 0), (4, 8, 8, 4, 1)),
    ("n128_z17", "bf16", 104, 32, K3, "z17", "NS NT S0", False, (8, 1, 4, 8, 2, 0, 0, 1, 0), (8, 8, 8, 8, 1)),
    ("w4_z17", "bf16", 104, 32, K3, "z17", "NS NT S0 NN", False, (4, 2, 4, 4, 2, 0, 0, 1, 0), (4, 8, 8, 8, 1)),
    ("tm3n32_z17", "bf16", 24, 32, K3, "z17", "NS S0", False, (8, 1, 3, 2, 2, 0, 0, 1, 0), (5, 9, 8, 2, 1)),
    ("tm3n128_z17", "bf16", 104, 32, K3, "z17", "NS S0", False, (8, 1, 3, 8, 2, 0, 0, 1, 0), (5, 9, 8, 8, 1)),
    ("sn32_z17", "bf16", 24, 32, K3, "z17", "NS NT", False, (8, 1, 4, 2, 2, 0, 0, 1, 1), (8, 8, 8, 2, 1)),
    ("sn32tm3_z17", "bf16", 24, 32, K3, "z17", "NS", False, (8, 1, 3, 2, 2, 0, 0, 1, 1), (5, 9, 8, 2, 1)),
    ("sn128_z17", "bf16", 104, 32, K3, "z17", "NS NT", False, (8, 1, 4, 8, 2, 0, 0, 1, 1), (8, 8, 8, 8, 1)),
    ("sn128tm3_z17", "bf16", 104, 32, K3, "z17", "NS", False, (8, 1, 3, 8, 2, 0, 0, 1, 1), (5, 9, 8, 8, 1)),
    ("sm32_z17", "bf16", 24, 32, K3, "z17", "S0", False, (2, 1, 4, 2, 2, 0, 0, 4, 0), (4, 4, 8, 2, 1)),
    ("sm_wk2_z17", "bf16", 104, 32, K3, "z17", "S0 M1", False, (2, 2, 4, 2, 2, 0, 0, 2, 0), (4, 4, 8, 4, 2)),
    ("sm_wk1_z17", "bf16", 200, 32, K3, "z17", "S0 M0", False, (2, 4, 4, 2, 2, 0, 0, 1, 0), (4, 4, 8, 8, 2)),
    ("ssm32_z17", "bf16", 24, 32, K3, "z17", "", False, (2, 1, 4, 2, 2, 0, 0, 4, 1), (4, 4, 8, 2, 1)),
    ("ssm_wk2_z17", "bf16", 104, 32, K3, "z17", "M1", False, (2, 2, 4, 2, 2, 0, 0, 2, 1), (4, 4, 8, 4, 2)),
    ("ssm_wk1_z17", "bf16", 200, 32, K3, "z17", "M0", False, (2, 4, 4, 2, 2, 0, 0, 1, 1), (4, 4, 8, 8, 2)),
    ("w5_z17", "bf16", 136, 32, K3, "z17", "NS", False, (4, 2, 4, 5, 2, 0, 0, 1, 0), (4, 8, 8, 10, 1)),
    ("w6_z17", "bf16", 168, 32, K3, "z17", "NS", False, (4, 2, 4, 6, 2, 0, 0, 1, 0), (4, 8, 8, 12, 1)),
    ("w7_z17", "bf16", 200, 32, K3, "z17", "NS", False, (4, 2, 4, 7, 2, 0, 0, 1, 0), (4, 8, 8, 14, 1)),
    ("w8_z17", "bf16", 232, 32, K3, "z17", "NS", False, (4, 2, 4, 8, 2, 0, 0, 1, 0), (4, 8, 8, 16, 1)),
    ("n144_z17s", "bf16", 144, 48, K5, "z17s", "NS", False, (8, 1, 4, 9, 2, 0, 0, 1, 0), (8, 8, 8, 9, 1)),
    # ---- ... and on the ten production levels ----------------------------------------------------------------------------
    ("n16_z10", "bf16", 8, 32, K3, "z10", "NS", False, (8, 1, 4, 1, 2, 0, 0, 1, 0), (7, 7, 10, 1, 1)),
    ("n32_z10", "bf16", 24, 32, K3, "z10", "NS NT S0", False, (8, 1, 4, 2, 2, 0, 0, 1, 0), (7, 7, 10, 2, 1)),
    ("n64_z10", "bf16", 40, 32, K3, "z10", "NS", False, (4, 1, 4, 4, 2, 0, 0, 1, 0), (5, 5, 10, 4, 1)),
    ("n128_z10", "bf16", 104, 32, K3, "z10", "NS NT S0", False, (8, 1, 4, 8, 2, 0, 0, 1, 0), (7, 7, 10, 8, 1)),
    ("w4_z10", "bf16", 104, 32, K3, "z10", "NS NT S0 NN", False, (4, 2, 4, 4, 2, 0, 0, 1, 0), (5, 5, 10, 8, 1)),
    ("tm3n32_z10", "bf16", 24, 32, K3, "z10", "NS S0", False, (8, 1, 3, 2, 2, 0, 0, 1, 0), (5, 7, 10, 2, 1)),
    ("tm3n128_z10", "bf16", 104, 32, K3, "z10", "NS S0", False, (8, 1, 3, 8, 2, 0, 0, 1, 0), (5, 7, 10, 8, 1)),
    ("sn32_z10", "bf16", 24, 32, K3, "z10", "NS NT", False, (8, 1, 4, 2, 2, 0, 0, 1, 1), (7, 7, 10, 2, 1)),
    ("sn32tm3_z10", "bf16", 24, 32, K3, "z10", "NS", False, (8, 1, 3, 2, 2, 0, 0, 1, 1), (5, 7, 10, 2, 1)),
    ("sn128_z10", "bf16", 104, 32, K3, "z10", "NS NT", False, (8, 1, 4, 8, 2, 0, 0, 1, 1), (7, 7, 10, 8, 1)),
    ("sn128tm3_z10", "bf16", 104, 32, K3, "z10", "NS", False, (8, 1, 3, 8, 2, 0, 0, 1, 1), (5, 7, 10, 8, 1)),
    ("sm32_z10", "bf16", 24, 32, K3, "z10", "S0", False, (2, 1, 4, 2, 2, 0, 0, 4, 0), (3, 4, 10, 2, 1)),
    ("sm_wk2_z10", "bf16", 104, 32, K3, "z10", "S0 M1", False, (2, 2, 4, 2, 2, 0, 0, 2, 0), (3, 4, 10, 4, 2)),
    ("sm_wk1_z10", "bf16", 200, 32, K3, "z10", "S0 M0", False, (2, 4, 4, 2, 2, 0, 0, 1, 0), (3, 4, 10, 8, 2)),
    ("ssm32_z10", "bf16", 24, 32, K3, "z10", "", False, (2, 1, 4, 2, 2, 0, 0, 4, 1), (3, 4, 10, 2, 1)),
    ("ssm_wk2_z10", "bf16", 104, 32, K3, "z10", "M1", False, (2, 2, 4, 2, 2, 0, 0, 2, 1), (3, 4, 10, 4, 2)),
    ("ssm_wk1_z10", "bf16", 200, 32, K3, "z10", "M0", False, (2, 4, 4, 2, 2, 0, 0, 1, 1), (3, 4, 10, 8, 2)),
    ("w5_z10", "bf16", 136, 32, K3, "z10", "NS", False, (4, 2, 4, 5, 2, 0, 0, 1, 0), (5, 5, 10, 10, 1)),
    # ---- bf16 with the LeakyReLU-backward mask -----------------------------------------------------------------------------
    ("m_n32_z17", "bf16", 24, 32, K3, "z17", "NS NT S0", True, (8, 1, 4, 2, 2, 1, 0, 1, 0), (8, 8, 8, 2, 1)),
    ("m_n64_z17", "bf16", 40, 32, K3, "z17", "NS", True, (4, 1, 4, 4, 2, 1, 0, 1, 0), (4, 8, 8, 4, 1)),
    ("m_w4_z17", "bf16", 104, 32, K3, "z17", "NS", True, (4, 2, 4, 4, 2, 1, 0, 1, 0), (4, 8, 8, 8, 1)),
    ("m_w5_z17", "bf16", 136, 32, K3, "z17", "NS", True, (4, 2, 4, 5, 2, 1, 0, 1, 0), (4, 8, 8, 10, 1)),
    ("m_w6_z17", "bf16", 168, 32, K3, "z17", "NS", True, (4, 2, 4, 6, 2, 1, 0, 1, 0), (4, 8, 8, 12, 1)),
    ("m_w7_z17", "bf16", 200, 32, K3, "z17", "NS", True, (4, 2, 4, 7, 2, 1, 0, 1, 0), (4, 8, 8, 14, 1)),
    ("m_tm3n32_z17", "bf16", 24, 32, K3, "z17", "NS S0", True, (8, 1, 3, 2, 2, 1, 0, 1, 0), (5, 9, 8, 2, 1)),
    ("m_sn32_z17", "bf16", 24, 32, K3, "z17", "NS NT", True, (8, 1, 4, 2, 2, 1, 0, 1, 1), (8, 8, 8, 2, 1)),
    ("m_sn32tm3_z17", "bf16", 24, 32, K3, "z17", "NS", True, (8, 1, 3, 2, 2, 1, 0, 1, 1), (5, 9, 8, 2, 1)),
    ("m_sm32_z17", "bf16", 24, 32, K3, "z17", "S0", True, (2, 1, 4, 2, 2, 1, 0, 4, 0), (4, 4, 8, 2, 1)),
    ("m_ssm32_z17", "bf16", 24, 32, K3, "z17", "", True, (2, 1, 4, 2, 2, 1, 0, 4, 1), (4, 4, 8, 2, 1)),
    ("m_n32_z10", "bf16", 24, 32, K3, "z10", "NS NT S0", True, (8, 1, 4, 2, 2, 1, 0, 1, 0), (7, 7, 10, 2, 1)),
    ("m_n64_z10", "bf16", 40, 32, K3, "z10", "NS", True, (4, 1, 4, 4, 2, 1, 0, 1, 0), (5, 5, 10, 4, 1)),
    ("m_w4_z10", "bf16", 104, 32, K3, "z10", "NS", True, (4, 2, 4, 4, 2, 1, 0, 1, 0), (5, 5, 10, 8, 1)),
    ("m_tm3n32_z10", "bf16", 24, 32, K3, "z10", "NS S0", True, (8, 1, 3, 2, 2, 1, 0, 1, 0), (5, 7, 10, 2, 1)),
    ("m_sn32_z10", "bf16", 24, 32, K3, "z10", "NS NT", True, (8, 1, 4, 2, 2, 1, 0, 1, 1), (7, 7, 10, 2, 1)),
    ("m_sn32tm3_z10", "bf16", 24, 32, K3, "z10", "NS", True, (8, 1, 3, 2, 2, 1, 0, 1, 1), (5, 7, 10, 2, 1)),
    ("m_sm32_z10", "bf16", 24, 32, K3, "z10", "S0", True, (2, 1, 4, 2, 2, 1, 0, 4, 0), (3, 4, 10, 2, 1)),
    ("m_ssm32_z10", "bf16", 24, 32, K3, "z10", "", True, (2, 1, 4, 2, 2, 1, 0, 4, 1), (3, 4, 10, 2, 1)),
    # ---- bf16, four taps of 8 channels (TPK 4): 24 reduction channels -----------------------------------------------------
    ("t4_n16_z17", "bf16", 8, 24, K3, "z17", "NS", False, (8, 1, 4, 1, 4, 0, 0, 1, 0), (8, 8, 8, 1, 1)),
    ("t4_n32_z17", "bf16", 24, 24, K3, "z17", "NS", False, (8, 1, 4, 2, 4, 0, 0, 1, 0), (8, 8, 8, 2, 1)),
    ("t4_n64_z17", "bf16", 40, 24, K3, "z17", "NS", False, (4, 1, 4, 4, 4, 0, 0, 1, 0), (4, 8, 8, 4, 1)),
    ("t4_n128_z17", "bf16", 104, 24, K3, "z17", "NS", False, (8, 1, 4, 8, 4, 0, 0, 1, 0), (8, 8, 8, 8, 1)),
    ("t4_w4_z17", "bf16", 104, 24, K3, "z17", "NS NN", False, (4, 2, 4, 4, 4, 0, 0, 1, 0), (4, 8, 8, 8, 1)),
    ("t4_w5_z17", "bf16", 136, 24, K3, "z17", "NS", False, (4, 2, 4, 5, 4, 0, 0, 1, 0), (4, 8, 8, 10, 1)),
    ("t4_w6_z17", "bf16", 168, 24, K3, "z17", "NS", False, (4, 2, 4, 6, 4, 0, 0, 1, 0), (4, 8, 8, 12, 1)),
    ("t4_w7_z17", "bf16", 200, 24, K3, "z17", "NS", False, (4, 2, 4, 7, 4, 0, 0, 1, 0), (4, 8, 8, 14, 1)),
    ("t4_w8_z17", "bf16", 232, 24, K3, "z17", "NS", False, (4, 2, 4, 8, 4, 0, 0, 1, 0), (4, 8, 8, 16, 1)),
    ("t4_n144_z17s", "bf16", 144, 24, K5, "z17s", "NS", False, (8, 1, 4, 9, 4, 0, 0, 1, 0), (8, 8, 8, 9, 1)),
    ("t4_n32_z10", "bf16", 24, 24, K3, "z10", "NS", False, (8, 1, 4, 2, 4, 0, 0, 1, 0), (7, 7, 10, 2, 1)),
    # ---- bf16, one tap of 32 channels (TPK 1): 1x1x1 convs the streaming kernel does not take --------------------------------
    ("t1_n16_z17", "bf16", 8, 64, K1, "z17", "", False, (8, 1, 4, 1, 1, 0, 0, 1, 0), (8, 8, 8, 1, 1)),
    ("t1_n32_z17", "bf16", 24, 64, K1, "z17", "", False, (8, 1, 4, 2, 1, 0, 0, 1, 0), (8, 8, 8, 2, 1)),
    ("t1_n64_z17", "bf16", 40, 64, K1, "z17", "", False, (4, 1, 4, 4, 1, 0, 0, 1, 0), (4, 8, 8, 4, 1)),
    ("t1_n128_z17", "bf16", 104, 64, K1, "z17", "", False, (8, 1, 4, 8, 1, 0, 0, 1, 0), (8, 8, 8, 8, 1)),
    ("t1_w4_z17", "bf16", 104, 64, K1, "z17", "NN", False, (4, 2, 4, 4, 1, 0, 0, 1, 0), (4, 8, 8, 8, 1)),
    ("t1_w5_z17", "bf16", 136, 64, K1, "z17", "", False, (4, 2, 4, 5, 1, 0, 0, 1, 0), (4, 8, 8, 10, 1)),
    ("t1_w6_z17", "bf16", 168, 64, K1, "z17", "", False, (4, 2, 4, 6, 1, 0, 0, 1, 0), (4, 8, 8, 12, 1)),
    ("t1_w7_z17", "bf16", 200, 64, K1, "z17", "", False, (4, 2, 4, 7, 1, 0, 0, 1, 0), (4, 8, 8, 14, 1)),
    ("t1_w8_z17", "bf16", 232, 64, K1, "z17", "", False, (4, 2, 4, 8, 1, 0, 0, 1, 0), (4, 8, 8, 16, 1)),
    ("t1_n144_z17s", "bf16", 144, 8192, K1, "z17s", "", False, (8, 1, 4, 9, 1, 0, 0, 1, 0), (8, 8, 8, 9, 1)),
    ("t1_n32_z10", "bf16", 24, 64, K1, "z10", "", False, (8, 1, 4, 2, 1, 0, 0, 1, 0), (7, 7, 10, 2, 1)),
    # ---- fp32 ---------------------------------------------------------------------------------------------------------------
    ("f_n16_z17", "fp32", 8, 32, K3, "z17", "", False, (8, 1, 4, 1, 2, 0, 1, 1, 0), (8, 8, 8, 1, 1)),
    ("f_n32_z17", "fp32", 24, 32, K3, "z17", "", False, (8, 1, 4, 2, 2, 0, 1, 1, 0), (8, 8, 8, 2, 1)),
    ("f_n64_z17", "fp32", 40, 32, K3, "z17", "", False, (4, 1, 4, 4, 2, 0, 1, 1, 0), (4, 8, 8, 4, 1)),
    ("f_n128_z17", "fp32", 104, 32, K3, "z17", "", False, (8, 1, 4, 8, 2, 0, 1, 1, 0), (8, 8, 8, 8, 1)),
    ("f_n144_z17", "fp32", 136, 32, K3, "z17", "", False, (8, 1, 4, 9, 2, 0, 1, 1, 0), (8, 8, 8, 9, 1)),
    ("f_w6_z17", "fp32", 168, 32, K3, "z17", "", False, (4, 2, 4, 6, 2, 0, 1, 1, 0), (4, 8, 8, 12, 1)),
    ("f_w8_z17", "fp32", 232, 32, K3, "z17", "", False, (4, 2, 4, 8, 2, 0, 1, 1, 0), (4, 8, 8, 16, 1)),
    ("f_t4_n16_z17", "fp32", 8, 12, K3, "z17", "", False, (8, 1, 4, 1, 4, 0, 1, 1, 0), (8, 8, 8, 1, 1)),
    ("f_t4_n32_z17", "fp32", 24, 12, K3, "z17", "", False, (8, 1, 4, 2, 4, 0, 1, 1, 0), (8, 8, 8, 2, 1)),
    ("f_t4_n64_z17", "fp32", 40, 12, K3, "z17", "", False, (4, 1, 4, 4, 4, 0, 1, 1, 0), (4, 8, 8, 4, 1)),
    ("f_t4_n128_z17", "fp32", 104, 12, K3, "z17", "", False, (8, 1, 4, 8, 4, 0, 1, 1, 0), (8, 8, 8, 8, 1)),
    ("f_t4_n144_z17", "fp32", 136, 12, K3, "z17", "", False, (8, 1, 4, 9, 4, 0, 1, 1, 0), (8, 8, 8, 9, 1)),
    ("f_m_n32_z17", "fp32", 24, 32, K3, "z17", "", True, (8, 1, 4, 2, 2, 1, 1, 1, 0), (8, 8, 8, 2, 1)),
    ("f_m_n64_z17", "fp32", 40, 32, K3, "z17", "", True, (4, 1, 4, 4, 2, 1, 1, 1, 0), (4, 8, 8, 4, 1)),
    ("f_m_w4_z17", "fp32", 104, 32, K3, "z17", "", True, (4, 2, 4, 4, 2, 1, 1, 1, 0), (4, 8, 8, 8, 1)),
    ("f_m_w5_z17", "fp32", 136, 32, K3, "z17", "", True, (4, 2, 4, 5, 2, 1, 1, 1, 0), (4, 8, 8, 10, 1)),
    ("f_n32_z10", "fp32", 24, 32, K3, "z10", "", False, (8, 1, 4, 2, 2, 0, 1, 1, 0), (7, 7, 10, 2, 1)),
    ("f_n128_z10", "fp32", 104, 32, K3, "z10", "", False, (8, 1, 4, 8, 2, 0, 1, 1, 0), (7, 7, 10, 8, 1)),
    ("f_w6_z10", "fp32", 168, 32, K3, "z10", "", False, (4, 2, 4, 6, 2, 0, 1, 1, 0), (5, 5, 10, 12, 1)),
    ("f_m_n32_z10", "fp32", 24, 32, K3, "z10", "", True, (8, 1, 4, 2, 2, 1, 1, 1, 0), (7, 7, 10, 2, 1)),
    ("f_m_w4_z10", "fp32", 104, 32, K3, "z10", "", True, (4, 2, 4, 4, 2, 1, 1, 1, 0), (5, 5, 10, 8, 1)),
    # ---- nothing forced, volumes of 128 and 64 levels: what the dispatcher's default route is ----------------------------------
    ("dflt_n32_big", "bf16", 24, 32, K3, "big", "", False, (8, 1, 4, 2, 2, 0, 0, 1, 1), (4, 8, 16, 2, 1)),
    ("dflt_n128_big", "bf16", 72, 32, K3, "big", "", False, (8, 1, 4, 8, 2, 0, 0, 1, 1), (4, 8, 16, 8, 1)),
    ("dflt_m_n32_big", "bf16", 24, 32, K3, "big", "", True, (8, 1, 4, 2, 2, 1, 0, 1, 1), (4, 8, 16, 2, 1)),
    ("dflt_n32_mid", "bf16", 24, 32, K3, "mid", "", False, (8, 1, 3, 2, 2, 0, 0, 1, 1), (3, 8, 16, 2, 1)),
    ("dflt_n128_mid", "bf16", 72, 32, K3, "mid", "", False, (8, 1, 3, 8, 2, 0, 0, 1, 1), (3, 8, 16, 8, 1)),
]

#: instantiations in the sources that no call reaches, with the check that keeps every call away.  Removal candidates.
UNREACHABLE = {
    (8, 1, 4, 1, 1, 0, 1, 1, 0): "fp32, TPK 1: TPK 1 needs a 1x1x1 conv, and both entry points return WSR_EUNSUPPORTED for "
                                 "`f32 && KX * KY * KZ == 1` (conv_tile.hip wsr_conv3d_fwd_tile / wsr_conv3d_dgrad_tile)",
    (8, 1, 4, 2, 1, 0, 1, 1, 0): "fp32, TPK 1: as above",
    (4, 1, 4, 4, 1, 0, 1, 1, 0): "fp32, TPK 1: as above",
    (8, 1, 4, 8, 1, 0, 1, 1, 0): "fp32, TPK 1: as above",
    (8, 1, 4, 9, 1, 0, 1, 1, 0): "fp32, TPK 1: as above",
}

INST_FIELDS = ("WM", "WN", "TM", "TN", "TPK", "MASK", "F32", "WK", "SIMPLE")


def ops():
    from gan_sr_wind_field_amd import hip_ops

    return hip_ops


@pytest.fixture(autouse=True)
def _no_launch_after_a_device_error():
    """a device error is sticky: end the session there instead of sending the remaining cases to a faulted device"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, no further launches: {e}", returncode=3)


def _bf(t):
    return t.bfloat16().float()


def f32s(v):
    """a scalar as the C side receives it"""
    return kb._f32(v)


class wsr_env:
    """WSR_* switches for the launches inside (``tags``: keys of SWITCHES), read again by the C side on entry and exit"""

    def __init__(self, monkeypatch, tags):
        self.mp, self.switches = monkeypatch, dict(SWITCHES[t] for t in tags.split())

    def __enter__(self):
        for name, v in self.switches.items():
            self.mp.setenv(name, str(v))
        reload_wsr_env()

    def __exit__(self, *exc):
        for name in self.switches:
            self.mp.delenv(name)
        reload_wsr_env()


# ---------------------------------------------------------------------------------------------------------------------
# operands, buffers, witness
# ---------------------------------------------------------------------------------------------------------------------

SPECIAL_BITS = {  # +0.0, -0.0, smallest positive / negative subnormal, smallest normal; a large negative value follows
    BF: (0x0000, 0x8000, 0x0001, 0x8001, 0x0080),
    F32: (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000),
}


def plant_specials(y, c_lo, c_hi):
    """``y``: saved output (B, C, X, Y, Z) of the test dtype on the host.  The special values go to the first voxel, a
    middle one and the last voxel of the last sample, at channels c_lo, c_lo + 1, ... and c_hi - 1, c_hi - 2, ...: the
    first and the last channels of a mask window that reads channels [c_lo, c_hi) of y."""
    B, _, X, Y, Z = y.shape
    iv = y.view(kb._INT_VIEW[y.dtype])
    bits = SPECIAL_BITS[y.dtype]
    wrap = 1 << (16 if y.dtype == BF else 32)
    for vx, vy, vz in ((0, 0, 0), (X // 2, Y // 2, Z // 2), (X - 1, Y - 1, Z - 1)):
        for i, b in enumerate(bits + (None,)):  # (windows narrower than the list take what fits)
            for c in (c_hi - 1 - i, c_lo + i):
                if not c_lo <= c < c_hi:
                    continue
                if b is None:
                    y[B - 1, c, vx, vy, vz] = -3.0e38
                else:
                    iv[B - 1, c, vx, vy, vz] = b - wrap if b >= wrap // 2 else b
    return y


@functools.lru_cache(maxsize=8)
def operands(N, R, k, vol, dtn, ups=False):
    """bf16-exact logical operands on the host, shared by every launch of a (widths, kernel, volume): forward conv
    R -> N (x, w, bias, res, cs) and input gradient of a conv N -> R (gy, wd, acc, ys, keep); never written to"""
    xyz, B = VOLUMES[vol]
    oxyz = (2 * xyz[0], 2 * xyz[1], xyz[2]) if ups else xyz
    dt = DT[dtn]
    gen = torch.Generator().manual_seed(100003 * N + 101 * R + 7 * k[0] + list(VOLUMES).index(vol))
    taps = math.prod(k)
    r = lambda *s: _bf(torch.randn(*s, generator=gen))
    op = dict(x=r((B, R) + xyz), w=_bf(torch.randn((N, R) + k, generator=gen) / math.sqrt(taps * R)), bias=r(N),
              res=r((B, N) + oxyz), cs=_bf(torch.rand((B, N), generator=gen) + 0.5),
              gy=r((B, R) + oxyz), wd=_bf(torch.randn((R, N) + k, generator=gen) / math.sqrt(taps * R)),
              acc=r((B, N) + oxyz), keep=_bf(torch.rand((B, N), generator=gen) + 0.5))
    op["keep"][0, 1] = op["keep"][B - 1, N - 3] = op["keep"][B - 1, N // 2] = 0.0
    op["ys"] = plant_specials(torch.randn((B, N) + oxyz, generator=gen).to(dt), 0, N)
    return op


def ndhwc(t, ctot, off, dt):
    """logical (B, C, X, Y, Z) host tensor -> the window [off, off + C) of an NDHWC device buffer, NaN elsewhere"""
    B, C_, X, Y, Z = t.shape
    buf = torch.full((B, X, Y, Z, ctot), NAN, dtype=dt, device=DEV)
    buf[..., off:off + C_] = t.permute(0, 2, 3, 4, 1).to(DEV).to(dt)
    return buf


def guarded(shape_bxyz, ctot, win, dt, fill=None):
    """guarded NDHWC buffer with the output window ``win`` = (off, C); ``fill``: a logical (B, C, X, Y, Z) host tensor"""
    f = None if fill is None else fill.permute(0, 2, 3, 4, 1).to(DEV).to(dt)
    return kb.Guarded(tuple(shape_bxyz) + (ctot,), dt, DEV, window=win, fill=f)


def plant(g, off, t):
    """put the logical tensor ``t`` into channels [off, off + C) of the guarded buffer, outside its output window: from
    here on those values are guard elements like the sentinel around them"""
    assert off >= g.win[0] + g.win[1] or off + t.shape[1] <= g.win[0]
    g.t[..., off:off + t.shape[1]] = t.permute(0, 2, 3, 4, 1).to(DEV).to(g.dtype)
    g.snap = g.base.view(kb._INT_VIEW[g.dtype])[g.mask].clone()


def logical(g):
    """the output window of a guarded NDHWC buffer as (B, C, X, Y, Z)"""
    return g.window_view().permute(0, 4, 1, 2, 3)


class witness:
    """``with witness(inst, plan, label):`` - the launch inside was served by the halo-tile kernel (the thread's launch
    count advanced by ``launches``), by the instantiation ``inst`` with the plan ``plan`` = (TX, TY, TZ, NTW, groups)
    [+ (ksplit,), default 1]"""

    def __init__(self, inst, plan, label, launches=1):
        self.inst, self.plan, self.label, self.launches = tuple(inst), tuple(plan), label, launches

    def __enter__(self):
        self.seq0 = ops().last_tile_instantiation()["seq"]
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        w, p = ops().last_tile_instantiation(), ops().last_tile_plan()
        print(f"[witness] {self.label}: {tuple(w[f] for f in INST_FIELDS)} seq +{w['seq'] - self.seq0} "
              f"plan {tuple(p[f] for f in ('TX', 'TY', 'TZ', 'NTW', 'ngroups', 'ksplit'))}")
        assert w["seq"] - self.seq0 == self.launches, \
            f"{self.label}: {w['seq'] - self.seq0} halo-tile launches, expected {self.launches} (another kernel served it?)"
        got = tuple(w[f] for f in INST_FIELDS)
        assert got == self.inst, f"{self.label}: instantiation {dict(zip(INST_FIELDS, got))}, expected {self.inst}"
        want = self.plan if len(self.plan) == 6 else self.plan + (1,)
        gotp = tuple(p[f] for f in ("TX", "TY", "TZ", "NTW", "ngroups", "ksplit"))
        assert gotp == want, f"{self.label}: plan {p}, expected (TX, TY, TZ, NTW, groups, ksplit) = {want}"
        return False


def slabs(vol):
    n = SLABBED.get(vol)
    if n is None:
        return [None]
    X = VOLUMES[vol][0][0]
    return [(0, n), (X - n, X)]


def _xs(t, xs):
    return t if xs is None or t is None else t[:, :, xs[0]:xs[1]]


def check(got, label, K, rho, vol, ref_fn):
    """``got`` (B, C, X, Y, Z) against ``ref_fn(xs) -> (ref, A)`` on every slab of the volume"""
    worst = 0.0
    for xs in slabs(vol):
        ref, A = ref_fn(xs)
        worst = max(worst, kb.assert_within(_xs(got, xs), ref, kb.bound(ref, A, K, rho), f"{label}{'' if xs is None else xs}"))
    assert worst <= 1.0
    return worst


def k_of(k, R, inst, extra=0):
    wk = inst[7]
    return math.prod(k) * R + (wk if wk > 1 else 0) + extra


# ---------------------------------------------------------------------------------------------------------------------
# the launches of an instantiation row
# ---------------------------------------------------------------------------------------------------------------------

def run_forward(rid, dtn, N, R, k, vol, inst, plan):
    """conv R -> N with bias + LeakyReLU + alpha + residual (a 1x1x1 conv also carries a channel scale, which keeps it
    off the streaming kernel)"""
    o, dt = ops(), DT[dtn]
    xyz, B = VOLUMES[vol]
    pad = tuple(kk // 2 for kk in k)
    op = operands(N, R, k, vol, dtn)
    one = k == K1
    xb = ndhwc(op["x"], R + 16, IN_OFF, dt)
    rb = ndhwc(op["res"], N + 16, 8, dt)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV), dtype=dt)
    g = guarded((B,) + xyz, N + 8, (OUT_OFF, N), dt)
    d = o.make_desc(o.ConvGeom(R, N, k, (1, 1, 1), pad), dt, B, xyz, R + 16, IN_OFF, N + 8, OUT_OFF)
    label = f"tile fwd {dtn}[{rid}]"
    cs = op["cs"] if one else None
    with witness(inst, plan, label):
        assert o.conv_fwd_tile(d, xb, wf, g.t, bias=op["bias"].to(DEV), act=True, slope=SLOPE, alpha=ALPHA, beta=BETA, res=rb,
                               res_off=8, chan_scale=None if cs is None else cs.to(DEV).contiguous(), use_ws=False) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    check(logical(g), label, k_of(k, R, inst), kb.rho_for(dt), vol,
          lambda xs: kb.ref_fwd(op["x"], op["w"], pad, bias=op["bias"], act=True, slope=f32s(SLOPE), chan_scale=cs,
                                alpha=f32s(ALPHA), res=_xs(op["res"], xs), beta=f32s(BETA), xs=xs))


def run_dgrad(rid, dtn, N, R, k, vol, inst, plan):
    """input gradient of a conv N -> R: dx (N channels) = alpha * conv^T(dy (R channels))"""
    o, dt = ops(), DT[dtn]
    xyz, B = VOLUMES[vol]
    pad = tuple(kk // 2 for kk in k)
    op = operands(N, R, k, vol, dtn)
    gb = ndhwc(op["gy"], R + 16, IN_OFF, dt)
    wt = o.pack_filter_frag(op["wd"].contiguous().to(DEV), transpose=True, dtype=dt)
    g = guarded((B,) + xyz, N + 8, (OUT_OFF, N), dt)
    d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, N + 8, OUT_OFF, R + 16, IN_OFF)
    label = f"tile dgrad {dtn}[{rid}]"
    with witness(inst, plan, label):
        assert o.conv_dgrad_tile(d, gb, wt, g.t, alpha=ALPHA, use_ws=False) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    check(logical(g), label, k_of(k, R, inst), kb.rho_for(dt), vol,
          lambda xs: kb.ref_dgrad(op["gy"], op["wd"], pad, alpha=f32s(ALPHA), xs=xs))


def dense_layout(N, R):
    """one buffer as the dense-block backward has it: dx window [8, 8 + N), dy window [dy_off, dy_off + R) behind it"""
    dy_off = (8 + N + 7) // 8 * 8 + 8
    return 8, dy_off, dy_off + R + 8


def run_masked_dgrad(rid, dtn, N, R, k, vol, inst, plan):
    """the growth-window launch of the dense-block backward (engine.py dgrad_dense): dx += conv^T(dy), times the
    LeakyReLU derivative of the saved output, in place - dx and dy are windows of one buffer, the saved output sits at
    dx's offset in a buffer of the same width"""
    o, dt = ops(), DT[dtn]
    xyz, B = VOLUMES[vol]
    pad = tuple(kk // 2 for kk in k)
    op = operands(N, R, k, vol, dtn)
    dx_off, dy_off, ctot = dense_layout(N, R)
    g = guarded((B,) + xyz, ctot, (dx_off, N), dt, fill=op["acc"])
    plant(g, dy_off, op["gy"])
    yb = ndhwc(op["ys"], ctot, dx_off, dt)  # (``ys`` has the test dtype: its planted bit patterns travel as they are)
    wt = o.pack_filter_frag(op["wd"].contiguous().to(DEV), transpose=True, dtype=dt)
    d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, ctot, dx_off, ctot, dy_off)
    label = f"tile masked dgrad {dtn}[{rid}]"
    with witness(inst, plan, label):
        assert o.conv_dgrad_tile(d, g.t, wt, g.t, alpha=1.0, accumulate=True, mask=(yb, dx_off, 0, N, MSLOPE),
                                 use_ws=False) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)  # (the dy window it read is part of the guard)
    check(logical(g), label, k_of(k, R, inst), kb.rho_for(dt), vol,
          lambda xs: kb.ref_dgrad(op["gy"], op["wd"], pad, acc=_xs(op["acc"], xs), mask_y=_xs(op["ys"], xs),
                                  slope=f32s(MSLOPE), mask_win=(0, N), xs=xs))


@pytest.mark.parametrize("row", INSTANTIATION_ROWS, ids=[r[0] for r in INSTANTIATION_ROWS])
def test_instantiation(hip, monkeypatch, row):
    rid, dtn, N, R, k, vol, tags, masked, inst, plan = row
    with wsr_env(monkeypatch, tags):
        if masked:
            run_masked_dgrad(rid, dtn, N, R, k, vol, inst, plan)
        else:
            run_forward(rid, dtn, N, R, k, vol, inst, plan)
            run_dgrad(rid, dtn, N, R, k, vol, inst, plan)


def test_rows_are_what_the_docstring_says():
    """the table itself: ragged n-tiles, ragged groups where there are groups, both level families, one row per default
    route, masked rows on masked instantiations only"""
    ids = [r[0] for r in INSTANTIATION_ROWS]
    assert len(set(ids)) == len(ids)
    for rid, dtn, N, R, k, vol, tags, masked, inst, plan in INSTANTIATION_ROWS:
        assert N == 144 or N % 16, rid
        assert bool(inst[5]) == masked and bool(inst[6]) == (dtn == "fp32"), rid
        assert plan[3] == inst[1] * inst[3], rid
        assert plan[4] == -(-(-(-N // 16)) // plan[3]), rid
        if plan[4] > 1:
            assert -(-N // 16) % plan[3], rid  # ragged last group
        xyz = VOLUMES[vol][0]
        assert math.prod(plan[:3]) <= inst[0] * inst[2] * 16, rid
        if vol in ("z17", "z17s", "z10"):
            for e, t in zip(xyz[:2], plan[:2]):
                assert e > t and e % t, rid  # two tiles at least and a ragged last one along x and y
        if vol in ("z17", "z17s"):
            assert xyz[2] > plan[2] and xyz[2] % plan[2], rid
    assert not set(r[8] for r in INSTANTIATION_ROWS) & set(UNREACHABLE)
    z10 = {r[8] for r in INSTANTIATION_ROWS if r[5] == "z10"}
    assert {i[:3] for i in z10} >= {(8, 1, 4), (8, 1, 3), (4, 1, 4), (4, 2, 4), (2, 1, 4), (2, 2, 4), (2, 4, 4)}


# ---------------------------------------------------------------------------------------------------------------------
# epilogue forms
# ---------------------------------------------------------------------------------------------------------------------

# carrier -> dtype, N, switches, and per (masked?, simple form allowed?) the instantiation and plan on volume z10
CARRIERS = {
    "n32_s1": ("bf16", 24, "NS NT S1"), "n32_s0": ("bf16", 24, "NS NT S0"),
    "n128_s1": ("bf16", 104, "NS NT S1"), "n128_s0": ("bf16", 104, "NS NT S0"),
    "wide": ("bf16", 136, "NS"),
    "f_n32": ("fp32", 24, ""), "f_n128": ("fp32", 104, ""), "f_wide": ("fp32", 136, ""),
}
EPI_R, EPI_VOL = 32, "z10"


def carrier_inst(name, masked, simple_ok):
    """the instantiation and plan a carrier's launch takes: masked or not, and whether the SIMPLE form may serve it"""
    dtn, N, tags = CARRIERS[name]
    f = int(dtn == "fp32")
    m = int(masked)
    s = int(simple_ok and "S1" in tags)
    if N == 24:
        return (8, 1, 4, 2, 2, m, f, 1, s), (7, 7, 10, 2, 1)
    if N == 104:
        if masked:
            return (4, 2, 4, 4, 2, 1, f, 1, 0), (5, 5, 10, 8, 1)
        return (8, 1, 4, 8, 2, 0, f, 1, s), (7, 7, 10, 8, 1)
    if masked:
        return (4, 2, 4, 5, 2, 1, f, 1, 0), (5, 5, 10, 10, 1)
    return ((8, 1, 4, 9, 2, 0, 1, 1, 0), (7, 7, 10, 9, 1)) if f else ((4, 2, 4, 5, 2, 0, 0, 1, 0), (5, 5, 10, 10, 1))


FWD_FORMS = ["bias", "res", "scale_act", "act_c1", "act2_inplace", "act2_c1", "scalar", "fmask0", "fmask16"]
DGRAD_FORMS = ["acc_all", "acc_n", "acc_src", "mask_sub", "mask_odd", "mask_keep", "planar"]
# (alpha != 1 without anything else, and the whole-window mask accumulated in place - the ``dgrad_dense`` launch of
# engine.py - are what every instantiation row runs)


def _fwd_cases():
    for c, (dtn, N, tags) in CARRIERS.items():
        for f in FWD_FORMS:
            if f.startswith("fmask") and dtn == "fp32":
                continue  # (declined: see test_declined_launch)
            yield f, c


def _dgrad_cases():
    for c in CARRIERS:
        for f in DGRAD_FORMS:
            yield f, c


@pytest.mark.parametrize("form,carrier", list(_fwd_cases()), ids=[f"{f}-{c}" for f, c in _fwd_cases()])
def test_forward_epilogue(hip, monkeypatch, form, carrier):
    o = ops()
    dtn, N, tags = CARRIERS[carrier]
    dt, k, pad, R, vol = DT[dtn], K3, (1, 1, 1), EPI_R, EPI_VOL
    xyz, B = VOLUMES[vol]
    op = operands(N, R, k, vol, dtn)
    c1 = 16 if N == 24 else 32  # act_c1: the growth width of the block
    masked = form.startswith("fmask")
    simple_ok = form not in ("scale_act", "scalar")
    inst, plan = carrier_inst(carrier, masked, simple_ok)
    xb = ndhwc(op["x"], R + 16, IN_OFF, dt)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV), dtype=dt)
    bias = op["bias"].to(DEV)
    out_off, ctot = (2, N + 6) if form == "scalar" else (OUT_OFF, N + 8)
    fill = op["res"] if form == "act2_inplace" else None
    g = guarded((B,) + xyz, ctot, (out_off, N), dt, fill=fill)
    d = o.make_desc(o.ConvGeom(R, N, k, (1, 1, 1), pad), dt, B, xyz, R + 16, IN_OFF, ctot, out_off)
    rb = ndhwc(op["res"], N + 16, 8, dt)
    kw, rk, extra = dict(bias=bias), dict(bias=op["bias"]), 0
    if form == "res":
        kw.update(alpha=ALPHA, beta=BETA, res=rb, res_off=8)
        rk.update(alpha=f32s(ALPHA), beta=f32s(BETA), res=op["res"])
    elif form == "scale_act":
        kw.update(act=True, slope=SLOPE, chan_scale=op["cs"].to(DEV).contiguous())
        rk.update(act=True, slope=f32s(SLOPE), chan_scale=op["cs"])
    elif form == "act_c1":  # first stage of the split dense-block forward (engine.py fwd_dense)
        kw.update(act=True, slope=SLOPE, act_c1=c1)
        rk.update(act=True, slope=f32s(SLOPE), act_c1=c1)
    elif form == "act2_inplace":  # second stage: the partial sums wait in the output window itself
        kw.update(act=2, slope=SLOPE, res=g.t, res_off=out_off, beta=1.0)
        rk.update(act2=True, slope=f32s(SLOPE), res=op["res"], beta=1.0)
        extra = 1
    elif form == "act2_c1":
        kw.update(act=2, slope=SLOPE, res=rb, res_off=8, beta=BETA, alpha=ALPHA, act_c1=c1)
        rk.update(act2=True, slope=f32s(SLOPE), res=op["res"], beta=f32s(BETA), alpha=f32s(ALPHA), act_c1=c1)
        extra = 1
    elif form == "scalar":  # an output window that starts at channel 2: vec_ok = 0, the scalar epilogue, with a residual
        kw.update(act=True, slope=SLOPE, alpha=ALPHA, beta=BETA, res=rb, res_off=8)
        rk.update(act=True, slope=f32s(SLOPE), alpha=f32s(ALPHA), beta=f32s(BETA), res=op["res"])
    elif masked:  # forward-form LeakyReLU-backward mask on [c0, N)
        c0 = 0 if form == "fmask0" else 16
        ys = plant_specials(op["ys"].clone(), c0, N)
        yb = ndhwc(ys, N + 16, 8, dt)
        kw.update(alpha=ALPHA, beta=BETA, res=rb, res_off=8, mask=(yb, 8 + c0, c0, N, MSLOPE))
        rk.update(alpha=f32s(ALPHA), beta=f32s(BETA), res=op["res"], mask_y=ys[:, c0:N], mask_win=(c0, N),
                  mask_slope=f32s(MSLOPE))
    label = f"tile fwd {dtn} {form}[{carrier}]"
    with wsr_env(monkeypatch, tags):
        with witness(inst, plan, label):
            assert o.conv_fwd_tile(d, xb, wf, g.t, use_ws=False, **kw) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    ref, A = kb.ref_fwd(op["x"], op["w"], pad, **rk)
    assert kb.assert_within(logical(g), ref, kb.bound(ref, A, 27 * R + extra, kb.rho_for(dt)), label) <= 1.0


@pytest.mark.parametrize("form,carrier", list(_dgrad_cases()), ids=[f"{f}-{c}" for f, c in _dgrad_cases()])
def test_input_gradient_epilogue(hip, monkeypatch, form, carrier):
    o = ops()
    dtn, N, tags = CARRIERS[carrier]
    dt, k, pad, R, vol = DT[dtn], K3, (1, 1, 1), EPI_R, EPI_VOL
    xyz, B = VOLUMES[vol]
    op = operands(N, R, k, vol, dtn)
    n_acc = 16 if N == 24 else 32
    masked = form.startswith("mask")
    simple_ok = form not in ("mask_odd", "mask_keep", "planar")
    inst, plan = carrier_inst(carrier, masked, simple_ok)
    wt = o.pack_filter_frag(op["wd"].contiguous().to(DEV), transpose=True, dtype=dt)
    dx_off, dy_off, ctot = dense_layout(N, R)
    kw, rk, extra, rho = dict(alpha=ALPHA), dict(alpha=f32s(ALPHA)), 0, kb.rho_for(dt)
    inplace = form in ("acc_all", "acc_n", "mask_sub", "mask_odd")
    if form == "planar":
        g = kb.Guarded((B, N) + xyz, F32, DEV)
        gb = ndhwc(op["gy"], R + 16, IN_OFF, dt)
        d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, N, 0, R + 16, IN_OFF)
        src, view, rho = gb, g.t, 0.0
        kw.update(dx_planar=True)
    elif inplace:  # dx and dy in two windows of one buffer; dx's window holds the accumulated value
        g = guarded((B,) + xyz, ctot, (dx_off, N), dt, fill=op["acc"])
        plant(g, dy_off, op["gy"])
        d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, ctot, dx_off, ctot, dy_off)
        src, view = g.t, logical(g)
    else:
        g = guarded((B,) + xyz, N + 8, (OUT_OFF, N), dt)
        gb = ndhwc(op["gy"], R + 16, IN_OFF, dt)
        d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, N + 8, OUT_OFF, R + 16, IN_OFF)
        src, view = gb, logical(g)
    if form == "acc_all":
        kw.update(accumulate=True)
        rk.update(acc=op["acc"], mask_win=None, acc_c1=N)
    elif form == "acc_n":
        kw.update(accumulate=n_acc)
        rk.update(acc=op["acc"], acc_c1=n_acc)
    elif form == "acc_src":  # the accumulated value comes from another tensor of dx's layout, with its own weight
        kw.update(accumulate=True, acc_src=ndhwc(op["acc"], N + 8, OUT_OFF, dt), acc_beta=ACC_BETA)
        rk.update(acc=op["acc"], acc_beta=f32s(ACC_BETA))
        extra = 1
    elif masked:
        c0, c1 = {"mask_sub": (16, N - 4), "mask_odd": (16, N - 2), "mask_keep": (0, N)}[form]
        ys = plant_specials(op["ys"].clone(), c0, c1)
        yb = ndhwc(ys, N + 16, 8, dt)
        keep = op["keep"] if form == "mask_keep" else None
        m = (yb, 8 + c0, c0, c1, MSLOPE) + (() if keep is None else (keep.to(DEV).contiguous(),))
        kw.update(mask=m)
        rk.update(mask_y=ys[:, c0:c1], mask_win=(c0, c1), slope=f32s(MSLOPE), keep=keep)
        if inplace:
            kw.update(accumulate=True)
            rk.update(acc=op["acc"])
    label = f"tile dgrad {dtn} {form}[{carrier}]"
    with wsr_env(monkeypatch, tags):
        with witness(inst, plan, label):
            assert o.conv_dgrad_tile(d, src, wt, g.t, use_ws=False, **kw) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    ref, A = kb.ref_dgrad(op["gy"], op["wd"], pad, **rk)
    assert kb.assert_within(view, ref, kb.bound(ref, A, 27 * R + extra, rho), label) <= 1.0


# ---- forms that belong to one instantiation ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtn,cout", [("bf16", 3), ("bf16", 15), ("fp32", 3), ("fp32", 15)])
def test_planar_forward_output(hip, monkeypatch, dtn, cout):
    """planar fp32 output (B, Cout, X, Y, Z) with Cout = 3 and 15: the scalar epilogue on a channel tail, <8,1,4,1>"""
    o, dt, k, pad, R, vol = ops(), DT[dtn], K3, (1, 1, 1), 32, "z10"
    xyz, B = VOLUMES[vol]
    op = operands(cout, R, k, vol, dtn)
    xb = ndhwc(op["x"], R + 16, IN_OFF, dt)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV), dtype=dt)
    g = kb.Guarded((B, cout) + xyz, F32, DEV)
    cp = o.pad_channels(cout, dt)
    d = o.make_desc(o.ConvGeom(R, cout, k, (1, 1, 1), pad), dt, B, xyz, R + 16, IN_OFF, cp, 0)
    label = f"tile fwd {dtn} planar[cout {cout}]"
    with wsr_env(monkeypatch, "NS"):
        with witness((8, 1, 4, 1, 2, 0, int(dtn == "fp32"), 1, 0), (7, 7, 10, 1, 1), label):
            assert o.conv_fwd_tile(d, xb, wf, g.t, bias=op["bias"].to(DEV), out_planar=True, use_ws=False) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    ref, A = kb.ref_fwd(op["x"], op["w"], pad, bias=op["bias"])
    assert kb.assert_within(g.t, ref, kb.bound(ref, A, 27 * R, 0.0), label) <= 1.0


@pytest.mark.parametrize("carrier", ["n32_s1", "n128_s1", "wide", "f_n128"])
def test_upsampled_forward(hip, monkeypatch, carrier):
    """nearest x(2, 2, 1) up-sampling folded into the halo load (no 384-voxel tiles, no SIMPLE form for it)"""
    o = ops()
    dtn, N, tags = CARRIERS[carrier]
    dt, k, pad, R, vol = DT[dtn], K3, (1, 1, 1), 32, "ups"
    xyz, B = VOLUMES[vol]
    oxyz = (2 * xyz[0], 2 * xyz[1], xyz[2])
    op = operands(N, R, k, vol, dtn, True)
    xb = ndhwc(op["x"], R + 16, IN_OFF, dt)
    rb = ndhwc(op["res"], N + 16, 8, dt)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV), dtype=dt)
    g = guarded((B,) + oxyz, N + 8, (OUT_OFF, N), dt)
    d = o.make_desc(o.ConvGeom(R, N, k, (1, 1, 1), pad, upsample=True), dt, B, xyz, R + 16, IN_OFF, N + 8, OUT_OFF)
    assert (d.Xo, d.Yo, d.Zo) == oxyz
    inst, _ = carrier_inst(carrier, False, False)
    ntw = inst[1] * inst[3]  # (14, 12, 10) voxels: 8x6x10 for the 512-voxel tiles, 2x12x10 for the 256-voxel ones
    plan = ((2, 12, 10) if ntw == 10 else (8, 6, 10)) + (ntw, 1)
    label = f"tile fwd {dtn} upsample[{carrier}]"
    with wsr_env(monkeypatch, tags):
        with witness(inst, plan, label):
            assert o.conv_fwd_tile(d, xb, wf, g.t, bias=op["bias"].to(DEV), act=True, slope=SLOPE, alpha=ALPHA, beta=BETA,
                                   res=rb, res_off=8, use_ws=False) is True, label
    torch.cuda.synchronize()
    kb.assert_guards_intact(g, label=label)
    ref, A = kb.ref_fwd(op["x"], op["w"], pad, ups=True, bias=op["bias"], act=True, slope=f32s(SLOPE), alpha=f32s(ALPHA),
                        res=op["res"], beta=f32s(BETA))
    assert kb.assert_within(logical(g), ref, kb.bound(ref, A, 27 * R, kb.rho_for(dt)), label) <= 1.0


TWO = {"bf16": (48, K5, 16, (8, 1, 4, 9, 2, 0, 0, 1, 0)), "fp32": (32, K3, 8, (8, 1, 4, 9, 2, 0, 1, 1, 0))}


@pytest.mark.parametrize("dtn", ["bf16", "fp32"])
def test_two_tensor_input_and_gradient(hip, monkeypatch, dtn):
    """the 144-wide form's two-tensor concat: ``in2`` (reduction channels >= c0 from a second tensor) forward, ``dx2``
    (produced channels >= 128 to a second tensor) in the input gradient"""
    o, dt, vol = ops(), DT[dtn], "z17s"
    R, k, c0, inst = TWO[dtn]
    N, pad = 144, tuple(kk // 2 for kk in k)
    xyz, B = VOLUMES[vol]
    op = operands(N, R, k, vol, dtn)
    plan = (8, 8, 8, 9, 1)
    xa = ndhwc(op["x"][:, :c0], c0 + 16, IN_OFF, dt)
    x2 = ndhwc(op["x"][:, c0:], R - c0 + 8, 0, dt)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV), dtype=dt)
    g = guarded((B,) + xyz, N + 8, (OUT_OFF, N), dt)
    d = o.make_desc(o.ConvGeom(R, N, k, (1, 1, 1), pad), dt, B, xyz, c0 + 16, IN_OFF, N + 8, OUT_OFF)
    label = f"tile fwd {dtn} in2"
    with wsr_env(monkeypatch, "NS"):
        with witness(inst, plan, label):
            assert o.conv_fwd_tile(d, xa, wf, g.t, bias=op["bias"].to(DEV), act=True, slope=SLOPE, in2=x2, in2_c0=c0,
                                   use_ws=False) is True, label
        torch.cuda.synchronize()
        kb.assert_guards_intact(g, label=label)
        ref, A = kb.ref_fwd(op["x"], op["w"], pad, bias=op["bias"], act=True, slope=f32s(SLOPE))
        assert kb.assert_within(logical(g), ref, kb.bound(ref, A, math.prod(k) * R, kb.rho_for(dt)), label) <= 1.0
        # input gradient of a conv 144 -> R: channels [0, 128) to dx, [128, 144) to channels [0, 16) of dx2
        gb = ndhwc(op["gy"], R + 16, IN_OFF, dt)
        wt = o.pack_filter_frag(op["wd"].contiguous().to(DEV), transpose=True, dtype=dt)
        g1 = guarded((B,) + xyz, 128 + 8, (OUT_OFF, 128), dt)
        g2 = guarded((B,) + xyz, 24, (0, 16), dt)
        dd = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, 128 + 8, OUT_OFF, R + 16, IN_OFF)
        label = f"tile dgrad {dtn} dx2"
        with witness(inst, plan, label):
            assert o.conv_dgrad_tile(dd, gb, wt, g1.t, alpha=ALPHA, dx2=g2.t, dx2_c0=128, use_ws=False) is True, label
        torch.cuda.synchronize()
        kb.assert_guards_intact(g1, g2, label=label)
        ref, A = kb.ref_dgrad(op["gy"], op["wd"], pad, alpha=f32s(ALPHA))
        got = torch.cat([logical(g1), logical(g2)], dim=1)
        assert kb.assert_within(got, ref, kb.bound(ref, A, math.prod(k) * R, kb.rho_for(dt)), label) <= 1.0


def test_split_reduction_keeps_to_the_general_form(hip, monkeypatch):
    """with a workspace, few workgroups and >= 4 chunks the SIMPLE form steps aside (conv_tile_impl.h :927) and the
    general one splits the reduction: 128 reduction channels on volume z17s -> 8 chunks over 12 tiles"""
    o, dt, k, pad, vol, N, R = ops(), BF, K3, (1, 1, 1), "z17s", 24, 128
    xyz, B = VOLUMES[vol]
    op = operands(N, R, k, vol, "bf16")
    xb = ndhwc(op["x"], R + 16, IN_OFF, dt)
    wf = o.pack_filter_frag(op["w"].contiguous().to(DEV), dtype=dt)
    d = o.make_desc(o.ConvGeom(R, N, k, (1, 1, 1), pad), dt, B, xyz, R + 16, IN_OFF, N + 8, OUT_OFF)
    ref, A = kb.ref_fwd(op["x"], op["w"], pad, bias=op["bias"], act=True, slope=f32s(SLOPE))
    for use_ws, inst, ks in ((True, (8, 1, 4, 2, 2, 0, 0, 1, 0), 4), (False, (8, 1, 4, 2, 2, 0, 0, 1, 1), 1)):
        g = guarded((B,) + xyz, N + 8, (OUT_OFF, N), dt)
        label = f"tile fwd bf16 split[ws {use_ws}]"
        with wsr_env(monkeypatch, "NS NT"):
            with witness(inst, (8, 8, 8, 2, 1, ks), label):
                assert o.conv_fwd_tile(d, xb, wf, g.t, bias=op["bias"].to(DEV), act=True, slope=SLOPE, use_ws=use_ws) is True
        torch.cuda.synchronize()
        kb.assert_guards_intact(g, label=label)
        assert kb.assert_within(logical(g), ref, kb.bound(ref, A, 27 * R + ks, kb.RHO_BF16), label) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# declined launches
# ---------------------------------------------------------------------------------------------------------------------

DECLINES = ["act2_no_res", "act2_planar", "act2_cout_mod4", "act2_mask_odd", "act2_mask_aligned", "fmask_fp32", "mask_dx_planar",
            "dx2_accumulate", "res2_3x3x3", "cout_gt_256", "mask_gt_224"]


@pytest.mark.parametrize("what", DECLINES)
def test_declined_launch(hip, monkeypatch, what):
    """False (or the argument error the header documents), a guarded output untouched bit for bit, no halo-tile launch"""
    o, dt, k, pad, vol = ops(), BF, K3, (1, 1, 1), "z10"
    xyz, B = VOLUMES[vol]
    N, R = {"act2_cout_mod4": (22, 32), "cout_gt_256": (264, 32), "mask_gt_224": (232, 32), "dx2_accumulate": (144, 48)}.get(what, (24, 32))
    if what == "fmask_fp32":
        dt = F32
    if what == "dx2_accumulate":
        k, pad = K5, (2, 2, 2)
    gen = torch.Generator().manual_seed(len(what))
    x = _bf(torch.randn((B, R) + xyz, generator=gen))
    w = _bf(torch.randn((N, R) + k, generator=gen) / math.sqrt(math.prod(k) * R))
    xb = ndhwc(x, R + 16, IN_OFF, dt)
    ctot = (N + 7) // 8 * 8 + 8
    res = ndhwc(_bf(torch.randn((B, N) + xyz, generator=gen)), ctot, OUT_OFF, dt)
    yb = ndhwc(_bf(torch.randn((B, N) + xyz, generator=gen)), ctot, 0, dt)
    planar = what in ("act2_planar", "mask_dx_planar")
    g = kb.Guarded((B, N) + xyz, F32, DEV) if planar else guarded((B,) + xyz, ctot, (OUT_OFF, N), dt)
    g2 = guarded((B,) + xyz, 24, (0, 16), dt)
    snap = [b.base.view(kb._INT_VIEW[b.dtype]).clone() for b in (g, g2)]
    before = o.last_tile_instantiation()
    fwd = what.startswith("act2") or what in ("fmask_fp32", "res2_3x3x3", "cout_gt_256")
    bias = torch.zeros(N, device=DEV)
    with wsr_env(monkeypatch, "NS"):
        if fwd:
            wf = o.pack_filter_frag(w.contiguous().to(DEV), dtype=dt)
            d = o.make_desc(o.ConvGeom(R, N, k, (1, 1, 1), pad), dt, B, xyz, R + 16, IN_OFF, N if planar else ctot,
                            0 if planar else OUT_OFF)
            kw = {"act2_no_res": dict(act=2), "act2_planar": dict(act=2, res=res, res_off=OUT_OFF, beta=1.0, out_planar=True),
                  "act2_cout_mod4": dict(act=2, res=res, res_off=OUT_OFF, beta=1.0),
                  "act2_mask_odd": dict(act=2, res=res, res_off=OUT_OFF, beta=1.0, mask=(yb, 0, 0, N - 2, MSLOPE)),
                  "act2_mask_aligned": dict(act=2, res=res, res_off=OUT_OFF, beta=1.0, mask=(yb, 0, 0, N, MSLOPE)),
                  "fmask_fp32": dict(mask=(yb, 0, 0, N, MSLOPE)),
                  "res2_3x3x3": dict(res=res, res_off=OUT_OFF, beta=1.0, res2=res, res2_off=OUT_OFF, beta2=1.0),
                  "cout_gt_256": dict(act=True)}[what]
            if what in ("act2_no_res", "act2_planar"):  # (the header's WSR_EINVAL: an argument error, not a shape to fall back from)
                with pytest.raises(RuntimeError):
                    o.conv_fwd_tile(d, xb, wf, g.t, bias=bias, use_ws=False, **kw)
            else:
                assert o.conv_fwd_tile(d, xb, wf, g.t, bias=bias, use_ws=False, **kw) is False, what
        else:
            wt = o.pack_filter_frag(_bf(torch.randn((R, N) + k, generator=gen) / 30).contiguous().to(DEV), transpose=True, dtype=dt)
            gb = ndhwc(_bf(torch.randn((B, R) + xyz, generator=gen)), R + 16, IN_OFF, dt)
            if what == "dx2_accumulate":
                d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, ctot, OUT_OFF, R + 16, IN_OFF)
                assert o.conv_dgrad_tile(d, gb, wt, g.t, accumulate=True, dx2=g2.t, dx2_c0=128, use_ws=False) is False
            elif what == "mask_dx_planar":
                d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, N, 0, R + 16, IN_OFF)
                with pytest.raises(RuntimeError):  # (WSR_EINVAL, as documented for a mask on a planar dx)
                    o.conv_dgrad_tile(d, gb, wt, g.t, dx_planar=True, mask=(yb, 0, 0, N, MSLOPE), use_ws=False)
            else:  # mask_gt_224: no masked instantiation is that wide
                d = o.make_desc(o.ConvGeom(N, R, k, (1, 1, 1), pad), dt, B, xyz, ctot, OUT_OFF, R + 16, IN_OFF)
                assert o.conv_dgrad_tile(d, gb, wt, g.t, mask=(yb, 0, 0, N, MSLOPE), use_ws=False) is False
    torch.cuda.synchronize()
    for b, s in zip((g, g2), snap):
        assert torch.equal(b.base.view(kb._INT_VIEW[b.dtype]), s), what
    assert o.last_tile_instantiation() == before, what


def test_calibration_table():
    """prints kb.WORST - the largest |err| / bound per label family seen by the cases above - for the test log; every
    entry was asserted <= 1 where it was produced"""
    fams = {}
    for label, worst in kb.WORST.items():
        if label.startswith("tile "):
            fams[label] = max(fams.get(label, 0.0), worst)
    for label in sorted(fams):
        print(f"[calibration] {label}: {fams[label]:.3g}")
    assert all(v <= 1.0 for v in fams.values())
