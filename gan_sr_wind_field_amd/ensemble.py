"""Geometric self-ensemble at test time ([ENSEMBLE]; the "+" variants of EDSR / ESRGAN): the generator runs on
transformed copies of its input, every output is mapped back, and the mapped outputs are averaged.  The training
augmentation (``data_aug_rot`` / ``data_aug_flip``) makes the generator approximately equivariant under the eight
symmetries of the square; the average cashes that in, and the spread between the members is a per-voxel uncertainty map.

A member is ``(k, fx)``, code ``k + 4 * fx``: ``k`` quarter turns as ``process_data._rotate_wind`` does them, then, if
``fx``, a mirror along x with u negated - the order of ``CustomizedDataset.__getitem__``.  Its inverse undoes the
mirror, then applies ``_rotate_wind(., (4 - k) % 4)``.  ``(2, 1)`` is the mirror along y.  The transforms and the
reduction are two HIP kernels (``csrc/ensemble.hip``): the wind-sign rules are stated there and nowhere else on the
evaluation path.
"""
from __future__ import annotations

from typing import Callable, List

import torch
from torch import Tensor

#: members -> [(k, fx)], in the order the members are stacked and summed
MEMBER_SETS = {
    1: [(0, 0)],
    2: [(0, 0), (0, 1)],
    4: [(0, 0), (2, 0), (0, 1), (2, 1)],  # no odd k: also for non-square domains
    8: [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1), (3, 1)],
}


def member_codes(members: int) -> List[int]:
    """the codes ``k + 4 * fx`` of a member set (1, 2, 4 or 8 members)"""
    if isinstance(members, bool) or members not in MEMBER_SETS:
        raise ValueError(f"members must be 1, 2, 4 or 8, not {members}")
    return [k + 4 * fx for k, fx in MEMBER_SETS[members]]


def _check_domain(members: int, X: int, Y: int) -> None:
    if members == 8 and X != Y:
        raise ValueError(f"members = 8 turns the domain by quarter turns and needs X == Y, not X = {X}, Y = {Y} "
                         "(members = 4 works on a non-square domain)")


def self_ensemble(fn: Callable[[Tensor, Tensor], Tensor], LR: Tensor, Z: Tensor, members: int = 8,
                  with_var: bool = False):
    """``fn`` averaged over a member set: the ``K`` transformed copies of ``LR`` (B, C, Xl, Yl, NZ; channels 0 and 1 the
    horizontal wind) and of the terrain tensor ``Z`` (B, 1, X, Y, NZ; a scalar) come from one launch each, ``fn`` is called
    ONCE on the stacked batch ``(K * B, ...)``, and its (K * B, 3, X, Y, NZ) output is mapped back and reduced in one
    launch.  -> ``mean`` (B, 3, X, Y, NZ), or ``(mean, var)`` with the population variance per component between the
    members."""
    codes = member_codes(members)
    _check_domain(members, LR.shape[2], LR.shape[3])
    _check_domain(members, Z.shape[2], Z.shape[3])
    from . import hip_ops

    K, B = len(codes), LR.shape[0]
    LR_m = hip_ops.dihedral_members(LR, codes, is_vector=True)
    Z_m = hip_ops.dihedral_members(Z, codes, is_vector=False)
    out = fn(LR_m.view((K * B,) + tuple(LR_m.shape[2:])), Z_m.view((K * B,) + tuple(Z_m.shape[2:])))
    if out.dim() != 5 or out.shape[0] != K * B or out.shape[1] != 3:
        raise ValueError(f"self_ensemble: fn returned {tuple(out.shape)} for a batch of {K} x {B}, wanted "
                         f"({K * B}, 3, X, Y, NZ)")
    out = out.detach().float().contiguous()
    return hip_ops.ensemble_reduce(out.view((K, B) + tuple(out.shape[1:])), codes, with_var=with_var)
