"""Element-wise error bounds for the conv kernels against float64 references, and guarded output buffers.

A plain helper module (like oracle_nets.py), imported by the kernel tests.

References
----------
``ref_fwd``, ``ref_dgrad`` and ``ref_wgrad`` evaluate the operation in float64 on the CPU
(``torch.nn.functional.conv3d`` / autograd) and return ``(ref, A)``: ``A`` is the same operation applied to
``|operands|`` (and ``|alpha|``, ``|beta|*|res|``, ``|bias|``, ``|mask|``) - the sum of the magnitudes of every term
that enters an element.  Tensors are logical: activations ``(B, C, X, Y, Z)``, filters ``(Cout, Cin, KX, KY, KZ)``.
``ref_pointwise`` is the voxel-local (1x1x1) operation with the streaming kernel's whole epilogue on ``(nvox, C)``
matrices: two residuals limited to the first ``res_c1`` produced channels and a LeakyReLU-backward mask on a channel
window.

The bound
---------
For every element

    |got - ref| <= rho * |ref|  +  lambda * sqrt(K) * 2^-24 * A  +  2^-100

* ``rho`` = 2^-8 when the kernel stores bf16 (round to nearest of an 8-bit significand), 0 for fp32 stores.  A result
  that is stored, read back and accumulated several times (``accumulate`` launches) pays rho once per stored value:
  pass the sum of their magnitudes as ``rho_mag``.
* ``K`` is the number of products in the element: taps * Cin (forward), taps * Cout (input gradient),
  B * voxels (filter gradient), plus ``n_parts`` for an ordered reduce of split copies or atomics.
* ``lambda`` = 16, one constant for every kernel and test (never tuned per test).

Ratios near 1 on bf16 outputs are expected, not a near-failure.  Rounding to bf16 moves a value by up to 2^-8 of
itself (half an ulp just above a power of two), and that is nearly all of the bound wherever the accumulation term is
small: the bf16 checks are in effect a half-ulp test of the stored result, measured at 0.97-0.99 of the bound on the
MI355X.  They are still sound - the fp32 accumulation error must fit the lambda term on top - and deterministic.  fp32
outputs and filter gradients (rho = 0) sit at a few hundredths of the bound or less.  Neither observation is a reason
to change lambda.

Why it holds.  The test operands are exact in bf16, so every product - bf16 x bf16 in the bf16 kernels, bf16-exact
fp32 x fp32 in the fp32 kernels - is exact in fp32.  The bf16 MFMAs add those exact products into fp32 accumulators;
the fp32 MFMA is a k-ordered ``fmaf`` chain.  Split partial sums, float atomics and the ordered reduce of split copies
are further fp32 additions, the epilogue (bias, alpha, beta * res, the LeakyReLU / Dropout3d scales) a few more
roundings.  Each of those roundings contributes at most 2^-24 times a partial sum, itself at most A.  The worst case
is gamma_K ~ K * 2^-24 * A; rounding errors of independent operands behave like a random walk, so the realistic bound
is C * sqrt(K) * 2^-24 * A, and lambda = 16 leaves a wide margin over C.  A bf16 store adds at most 2^-8 of the stored
value.  LeakyReLU is 1-Lipschitz, so an error in front of it passes through at most unchanged.  The 2^-100 only keeps
the bound positive where ref and A are both zero.

The streaming 1x1x1 kernel (``ref_pointwise``, K = reduction channels + 3) starts its accumulators from
bias + (beta / alpha) * res + (beta2 / alpha) * res2 and multiplies by alpha at the end: the quotient and the final
product are two more fp32 roundings of terms that A already contains, which is what the "+ 3" pays for.  Its in-place
and accumulating forms still store each element once - the accumulated values are read as exact bf16 operands, like
any residual - so rho is paid once, on |ref|.

The stride-1 halo-tile kernel (``ref_fwd`` / ``ref_dgrad`` with their further forms; K = taps * reduction channels) adds
to K: ``WK`` where WK > 1 waves share the K-steps of a stage and their partial sums meet in LDS (WK - 1 more fp32
additions of partial sums, each at most A), ``ksplit`` where the reduction is split over workgroups, and 1 where a
residual joins the sum in front of the activation (``act2``) or an accumulated value comes from another tensor with its
own weight (``acc_src`` / ``acc_beta``): one more product and one more addition of a term A already holds.  The mask
and channel-scale factors are exact selections or single roundings inside the lambda term.  An accumulate that reads
back a value the kernel itself stored earlier pays rho for it through ``rho_mag``; one that reads a test operand (exact
in bf16, like any residual) does not.

BatchNorm (``ref_bn_*``; test_batchnorm_matrix.py).  Every stage is referenced from the fp32 tables the kernel itself
receives - shift, mean, invstd, gamma, beta, sums, inv_n, scalars through ``_f32`` - so the stages are isolated and no
error compounds; activations are bf16-exact in the bf16 rows.  The same bound with these K:

* the reductions ``ref_bn_sums`` {sum d, sum d^2} and ``ref_bn_bwd_sums`` {sum g', sum g' xhat}: K = nvox + rows,
  rho = 0 - nvox additions of terms plus the ``rows`` partial rows of the final kernel (the workgroups' atomics in the
  scalar kernels).  A term costs at most three roundings of itself (x - shift, the product, (x - mean) * invstd), 3u of a
  magnitude A already holds: inside the lambda term for every K >= 1.
* the dy that ``bn_bwd_reduce`` writes back, ``ref_bn_bwd_dy``: one product, K = 1, rho of the stored type; bit-identical
  to its input where the mask is 1.
* ``ref_bn_finalize``: var = max(s2 / cnt - dm^2, 0) is three roundings with contraction off (two quotients' worth of
  s2 / cnt and dm^2, one difference; max is 1-Lipschitz): ``bound(var, A_var, 3, 0)`` with A_var = s2 / cnt + dm^2.
  invstd = (var + eps)^-1/2 turns an error e of var into invstd * e / (2 (var + eps)); var + eps and ``rsqrtf`` add
  two relative roundings, the LAMBDA * 2^-24 term.  rm = (1 - m) rm0 + m mean: K = 3 (two products, one sum; 1 - m is a
  rounding of a factor); rv the same with unb = var * (cnt / max(cnt - 1, 1)) in it, two more: K = 5, A with A_var.
  After G ordered updates (``ref_bn_running``) K = 3G and 5G on the running sum of term magnitudes.  ``bn_mean``: one
  quotient, K = 1.  ``bn_train_stats`` keeps its sums on the device: its mean is held to ``ref_bn_sums / cnt`` with
  K = nvox + rows + 1 (the quotient), its invstd and running statistics to ``ref_bn_finalize`` / ``ref_bn_running`` of
  the float64 sums of x shifted by the mean it wrote, with the SAME bounds as above (K = 3 inside invstd, 3G and 5G)
  and nothing added for the fp32 sums in between: their error is a random walk over nvox terms of a sum that is
  divided by cnt, far inside the lambda term (measured below), and a wider bound would let a ``cnt`` off by one
  through at 25603 voxels.
* ``ref_bn_apply``: x - mean, two products, one sum: K = 4, rho of the stored type.
* ``ref_bn_bwd_apply``: the mask product, sums * inv_n, xhat (two), its product with sums * inv_n (two), two
  differences and the product with gamma * invstd (two) - ten roundings at most in either kernel's order, of three
  terms whose magnitudes A sums: K = 8 (10 u A < LAMBDA sqrt(8) u A) covers the one-element kernel and the 8-wide
  one.

Worst |err| / bound per label of test_batchnorm_matrix.py on the MI355X (its ``[bound]`` lines; bf16 rows / fp32 rows):
bn_stats 0.037 / 0.029, shifted 0.009 / 0.025; bn_bwd_reduce sums 0.016 / 0.020 (act off 0.003 / 0.004), its
written-back dy 0.79 / 0.059; bn_mean 0.061; bn_finalize invstd 0.067, running mean 0.078, running var 0.062;
bn_train_stats mean 0.001 / 0.005, invstd 0.106 / 0.107, running mean 0.065 / 0.076, running var 0.063 / 0.057 (the
largest at (2, 512, 16421); the fp32 emulation of the fused chain on the CPU reaches 0.08); bn_apply 0.995 / 0.077;
bn_bwd_apply, one-element kernel, 0.995 / 0.088 over the four forms, 0.995 on the two one-element routes of the big
data; bn_bwd_apply_v8 0.995 (sums), 0.994 (act_y), 0.995 (both).  As everywhere in this module: a bf16 store sits at
the half-ulp limit, fp32 results at a few hundredths; the written-back bf16 dy at 0.79 because dy * 0.2 of an 8-bit
significand seldom lands near a rounding tie.  No row exceeded its bound.

The network boundary (``ref_deriv`` .. ``ref_plane_sum``; test_boundary_matrix.py): the content loss of the generator,
the wind gradient and the planar fp32 <-> NDHWC kernels, every stage from the fp32 operands the kernel receives, rho = 0
throughout (fp32 stores; the copies are compared as bit patterns, bf16 copies with the host's round-to-nearest-even).

* one derivative element (``ref_deriv``, ``ref_wind_gradient``): K_STENCIL = 12, the longest chain of roundings into
  one term, counted in ``deriv_row`` (stencil.h :18-20) and ``jacobian``: hl and hr (two differences), hr * hr and
  hl * hl (two products), their difference, hl * hr, hl + hr and their product (den, three), the quotient, the product
  with f_i, two additions of the three terms - 2 + 2 + 1 + 3 + 1 + 1 + 2.  The chain through a or c is one shorter, the
  one-sided rows have four.  A = |a| |f-| + bmag |f_i| + |c| |f+| with bmag = (hr^2 + hl^2) / |den|, the centre
  weight's magnitude BEFORE hr^2 - hl^2 cancels: the roundings of the two squares are relative to the squares, not to
  their difference.  With |b| |f_i| instead, the fp32 emulation of the same correct arithmetic leaves the bound 124-fold
  on the grid 100.37 i + 1e-5 i^1.5 at a centre value of 1e6 (746-fold when the difference of the squares is contracted
  into one fma, which then returns the rounding error of hl * hl where hr == hl) and stays at 0.04 of it with bmag
  (test_kernel_bounds.py).  On 100 i + 1e-5 i^1.5 itself the fp32 spacings are 100 or 100 + 2^-13, whose squares are
  exact, and both forms hold.
* the adjoint (``ref_wind_gradient_bwd``): K_ADJOINT = 19 - the nine roundings of a centre weight, the product, and
  the nine additions into ``acc`` over the three axes; A the same expression on magnitudes with bmag.
* the residual (``ref_physics_residual``): K_RESIDUAL = 23 - a Jacobian entry (12), J_sr - J_hr and the product with
  2 coef (2; the doubling is exact), and on channels 0, 4, 8 the divergence route: d2 (three), d3 (two), g2 * d3, g3 * d2
  and their sum (three), the addition into o (one).  A = 2 |coef| (M_sr + M_hr) per route.
* dsr (``ref_physics_adjoint``): K_DSR = 24 - the adjoint's 19, SR - HR, coef[4] * sign, 2 coef[5] * d, their sum and
  the addition into ``acc``; referenced from the residual the first launch wrote.
* the six sums of ``ref_physics_stats``: K = terms + rows + per-term roundings, terms = {6, 3, 1, 1, 3, 3} * voxels,
  rows = ``physics_rows``, per-term = 27 for the Jacobian sums (two entries of 12, their difference, twice through
  the square, the product), 31 and 29 for the divergences (+ 2, + 1 additions on either side), 1 and 3 for sum |d| and
  sum d^2; A = sum (M_sr + M_hr)^2.  Where SR is close to HR that A is 10^4 times the sum, so the four Jacobian sums
  are also held to a narrower bound that follows the element bounds through the square (``tight_sums``).  The eight
  maxima: the largest element bound in the range (max is 1-Lipschitz); NaN where the range holds one.
* ``ref_zfold``: K = KZ + 1, A = |bias| + sum |t|.  ``ref_plane_sum``: K = B V + rows, rows = ``plane_sum_rows``.

Worst |err| / bound per label of test_boundary_matrix.py on the MI355X: wind_gradient 0.033, wind_gradient_bwd 0.048;
physics_stats 0.019 over the main rows (0.022 with every z-derivative negative, 0.022 with a spike, 0.016 of the HR
maxima beside a NaN), its four Jacobian sums against the narrower bound 0.005; physics_residual 0.011 (one-hot 0.011),
physics_adjoint 0.032 (one-hot 0.050, coef[0..3] = 0 with equal levels 0.012); zfold 0.061; plane_sum 0.0019; through
the wrappers wind_gradient 0.020 and 0.034 backward, physics_loss_stats 0.002 and 0.017 backward, zfold 0.041,
plane_sum 4e-5.  Every copy row (planar_to_ndhwc, ndhwc_to_planar, zunfold, fp32 and bf16) and every pixel-term row
matched bit for bit: 0.  The fp32 emulations on the CPU reach 0.038 (Jacobian), 0.040 (adjoint), 0.040 (residual),
0.045 (dsr), 0.015 (statistics).  No row exceeded its bound.

The table Adam family (``ref_adam`` .. ``clip_coef``; test_optimizer_matrix.py): ``torch.optim.Adam``'s definition - L2
weight decay, both bias corrections, eps outside the root - in float64 from the fp32 p, g, m, v the kernel receives and
the hyper-parameters as Python doubles, rho = 0.  The bounds are propagated through ``adam_one`` (elementwise.hip :618)
the way ``bn_finalize_bounds`` does it, not one (A, K) term:

* m' = beta1 m + (1 - beta1)(g + wd p): K = 5 - wd p, the sum with g, the product with 1 - beta1, beta1 m, the sum -
  on A_m = beta1 |m| + (1 - beta1)(|g| + wd |p|).  The eight ``AdamK`` constants (``adam_k`` :608) are doubles rounded
  once: relative perturbations of factors A already holds.  They are counted in K: three of them (wd, 1 - beta1, beta1)
  enter m', so the worst case is 8 u A_m, against LAMBDA sqrt(5) u A_m = 35.8 u A_m.
* v' = beta2 v + (1 - beta2)(g + wd p)^2: K = 6 (the same plus the second product with g) on A_v, the same expression
  on magnitudes - every term is non-negative, and A_v = v' unless g and wd p cancel.  Constants: wd twice, 1 - beta2,
  beta2; worst case 10 u A_v against 39.2 u A_v.
* the denominator sqrt(v') / sqrt(bc2) + eps takes v's bound through the root, |sqrt(v' + e) - sqrt(v')| over |e| <=
  bound_v evaluated exactly (bound_v / (2 sqrt v') to first order, sqrt(bound_v) at v' = 0, and no blow-up between the
  two), divided by sqrt(bc2), plus three relative roundings - the root, the quotient, the sum with eps - as
  LAMBDA sqrt(3) u denom (the rounded sqrt(bc2) and eps are two more relative perturbations inside that term).
* the quotient m' / denom: (bound_m + (A_m / denom) bound_denom) / (denom - bound_denom) - the first-order
  bound_m / denom + (A_m / denom) relerr(denom) with the exact divisor - plus one rounding, LAMBDA u A_m / denom.
* p' = p - step_size * that: step_size times the quotient's bound, plus K = 3 (the product, the difference, the
  rounded step_size) on |p| + step_size A_m / denom.
* with clipping (``coef``) the gradient is coef * g, rounded three times on its way (``K_CLIP_G``: total + 1e-6, the
  quotient, the product): the written-back g' has K = 3 on |coef g|, and m' and v' take 3 and 6 more in K.  coef itself
  is ``clip_coef``: float64 from the fp32 total the kernel wrote.
* ``ref_grad_sqnorm``: K = n + 10, A the sum.  ``ref_clip_total``: the float64 root of the sum of the fp32 partials the
  first launch wrote, K = n_jobs + 2 (the kernel adds in double and rounds the root once).
* |g| = 1e-25: g^2 is zero in fp32 and 1e-50 in the reference; 2^-100 = 8e-31 covers the difference in v', and
  sqrt(2^-100) = 9e-16 is nothing beside eps = 1e-8 in the denominator (test_kernel_bounds.py asserts both).

The single-tensor entry ``wsr_adam_step`` (``adam_kernel`` :590) receives its hyper-parameters as fp32 and takes
``1.f - beta2`` in fp32 (:597) - exact for the float it holds, but 1 - float(0.999) is 1.3e-5 (relative) off
1 - 0.999: against the double hyper-parameters its exp_avg_sq leaves the bound 5.6-fold (test_kernel_bounds.py,
``one_minus_beta2_in_fp32``).  It is therefore referenced from the fp32 values it receives (``f32_hyper``), where it
sits where the table kernels sit; the table entry points take doubles and round 1 - beta once.  INTEGRATION.md says
the same in the entry's row.

Worst |err| / bound per label of test_optimizer_matrix.py on the MI355X beside the fp32 emulation on the CPU
(test_kernel_bounds.py, in brackets): adam_multi p 0.039 [0.037], exp_avg 0.070 [0.075], exp_avg_sq 0.116 [0.114];
adam_multi_clip p 0.036 [0.035], exp_avg 0.065 [0.064], exp_avg_sq 0.099 [0.070 on one tensor of 1027 elements; the
launches cover 170 000 elements per row], its written-back g 0.051, total 0.0087 (0.0092 over the job counts 1 .. 600);
grad_sqnorm_multi partials 0.029 (small jobs 0.036, with a spike 0.033); adam_step p 0.038, exp_avg 0.067, exp_avg_sq
0.103; TableAdam.step over three steps p 0.036, exp_avg 0.067, exp_avg_sq 0.102, g 0.069, norm 0.001.  The shadow of
the moving average against test_ema.py's ``step_bound`` (3 u, a worst-case count, not a LAMBDA bound) 0.72, as
test_ema_gpu.py measures it.  As expected for fp32 results: a few hundredths to a tenth of the bound, and no label's
GPU ratio above one and a half times its emulation's.  No row exceeded its bound.

The glue of the backward pass (``ref_lrelu_bwd`` .. ``ref_chan_sum_partials``; test_glue_matrix.py), operands exact in
bf16, rho of the stored type:

* ``ref_lrelu_bwd``: g * (y > 0 ? 1 : slope) * chan_scale: K = 2 - slope * scale, then the product with g; where the
  whole factor is 1 the element is returned bit for bit, a keep factor of 0 gives a zero of g's sign.
* ``ref_chan_axpby``: alpha * src + beta * dst: K = 3 (two products, one sum), rho once; beta == 0 does not read dst.
* ``ref_upsample2_bwd``: three additions, K = 3, A the sum of the four magnitudes.
* ``ref_chan_sum``: K = nvox + rows (``chan_sum_geometry``), rho = 0, A = |scale| sum |x|; a row of the partial table
  (``ref_chan_sum_partials``) K = ceil(nvox / rows) + lanes.  The engine's form - the partial rows reduced by
  ``wsr_unpack_wgrad_reduce_multi`` - the same K = nvox + rows.

Worst |err| / bound per label of test_glue_matrix.py on the MI355X (bf16 rows / fp32 rows; the CPU emulation in
brackets): lrelu_bwd 0.966 / 0.044; chan_axpby 0.79 / 0.034 with beta = 0 (alpha * s of an 8-bit significand seldom
lands near a tie) and 0.996 / 0.036 with beta on; upsample2_bwd 0.996 / 0.097; chan_sum 0.037 / 0.024 [0.035] at scale
0.2 - the one-voxel row, where the product with the scale is the only rounding - and 0.001 / 0.005 [0.004] at scale 1
(bf16-exact operands add without rounding until the sum outgrows 24 bits), its partial rows 0.012 / 0.058, with a spike
0.001 / 0.002, the engine's form 0.001 / 0.001.  bf16 stores at the half-ulp limit, fp32 results at a few hundredths.
No row exceeded its bound.

A kernel bug that drops one tap at one voxel, loses one split or misplaces one channel chunk changes the elements it
touches by a sizable fraction of A / sqrt(K), far above the bound; a whole-tensor relative L2 check averages such an
error over every element and can miss it.

Guarded buffers
---------------
``Guarded`` allocates a tensor as a view inside a larger allocation.  The guard bands before and after it, and the
channels outside the channel window the kernel may write, hold a sentinel (a NaN payload for fp32, a fixed finite
pattern for bf16); ``assert_guards_intact`` compares them bit for bit.
"""
import math

import torch
import torch.nn.functional as F

LAMBDA = 16.0
U_FP32 = 2.0 ** -24
RHO_BF16 = 2.0 ** -8
TINY = 2.0 ** -100


def rho_for(dt) -> float:
    """rho of a kernel that stores ``dt``"""
    return RHO_BF16 if dt == torch.bfloat16 else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------

def _d(t):
    return None if t is None else t.detach().to(torch.float64).cpu()


def up2(x):
    """nearest x(2,2,1) up-sampling of (B, C, X, Y, Z)"""
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def fold2(x):
    """adjoint of ``up2``: sum of each 2 x 2 block in x-y"""
    B, C, X, Y, Z = x.shape
    return x.reshape(B, C, X // 2, 2, Y // 2, 2, Z).sum(dim=(3, 5))


def _win(t, win):
    return t if win is None else t[:, win[0]:win[0] + win[1]]


def _conv_slab(x, w, pad, xs, stride=(1, 1, 1)):
    """conv3d of x (B, C, X, Y, Z) with zero padding ``pad`` and output stride ``stride``; ``xs`` = (x0, x1): only
    output x-planes [x0, x1) (the input slab they read plus its halo)"""
    stride = tuple(stride)
    if xs is None:
        return F.conv3d(x, w, None, stride, tuple(pad))
    kx = w.shape[2]
    xp = F.pad(x, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    return F.conv3d(xp[:, :, xs[0] * stride[0]:(xs[1] - 1) * stride[0] + kx], w, None, stride, 0)


def _lrelu_mask(mask_y, slope):
    """(y > 0 ? 1 : slope) of a saved output in float64: -0.0, +0.0 and every negative value take ``slope``, every
    positive value - subnormals included - takes 1"""
    return torch.where(_d(mask_y) > 0, 1.0, float(slope)).to(torch.float64)


def _apply_mask(v, a, mask_y, mask_win, mask_slope):
    """columns ``mask_win`` = [c0, c1) (default: all) of v and a times ``_lrelu_mask(mask_y)``; mask_y has c1 - c0
    channels"""
    m = _lrelu_mask(mask_y, mask_slope)
    c0, c1 = (0, v.shape[1]) if mask_win is None else mask_win
    assert 0 <= c0 < c1 <= v.shape[1] and m.shape == v[:, c0:c1].shape, (tuple(m.shape), tuple(v.shape), mask_win)
    v, a = v.clone(), a.clone()
    v[:, c0:c1] *= m
    a[:, c0:c1] *= m.abs()
    return v, a


def ref_fwd(x, w, pad, *, ups=False, bias=None, act=False, slope=0.2, chan_scale=None, alpha=1.0, res=None, beta=0.0,
            in_win=None, xs=None, stride=(1, 1, 1), act_c1=None, act2=False, mask_y=None, mask_win=None,
            mask_slope=0.2):
    """y = alpha * s * lrelu(conv(up?(x), w) + bias) + beta * res  (the forward epilogue order of ``wsr_epilogue_t``).
    ``in_win`` = (off, C): channels of x that enter; ``chan_scale`` (B, Cout); ``xs``: output x-planes [x0, x1) only
    (``res`` then covers those planes); ``stride``: the conv's output stride (the discriminator's down-sampling convs).

    The halo-tile kernel's further forms (its epilogue, conv_tile_impl.h :679-713, in the kernel's own order
    ``(acc + bias) -> act -> * (chan_scale * alpha) -> + beta * res -> * mask``):

    * ``act_c1``: bias and LeakyReLU on produced channels below ``act_c1`` only, raw conv sums on the rest (the first
      stage of a split dense-block conv);
    * ``act2=True`` (``wsr_epilogue_t.act = 2``, the second stage): the residual joins BEFORE the activation,
      ``alpha * s * lrelu(conv + bias + beta * res)`` below ``act_c1`` and ``alpha * s * (conv + beta * res)`` from
      ``act_c1`` on (:679-690);
    * ``mask_y`` / ``mask_win`` = (c0, c1) / ``mask_slope``: the forward-form LeakyReLU-backward mask
      (``wsr_epilogue_t.mask``), applied last: channels [c0, c1) times (mask_y > 0 ? 1 : mask_slope), ``mask_y`` holding
      c1 - c0 channels.

    With none of the three given the result is what it always was, bit for bit.  Returns (ref, A)."""
    if act_c1 is not None or act2 or mask_y is not None:
        return _ref_fwd_forms(x, w, pad, ups=ups, bias=bias, act=act, slope=slope, chan_scale=chan_scale, alpha=alpha,
                              res=res, beta=beta, in_win=in_win, xs=xs, stride=stride, act_c1=act_c1, act2=act2,
                              mask_y=mask_y, mask_win=mask_win, mask_slope=mask_slope)
    x, w = _win(_d(x), in_win), _d(w)
    if ups:
        x = up2(x)
    v = _conv_slab(x, w, pad, xs, stride)
    a = _conv_slab(x.abs(), w.abs(), pad, xs, stride)
    if bias is not None:
        b = _d(bias).view(1, -1, 1, 1, 1)
        v, a = v + b, a + b.abs()
    if act:
        v = F.leaky_relu(v, slope)
    if chan_scale is not None:
        s = _d(chan_scale).view(v.shape[0], v.shape[1], 1, 1, 1)
        v, a = v * s, a * s.abs()
    v, a = alpha * v, abs(alpha) * a
    if res is not None:
        r = _d(res)
        v, a = v + beta * r, a + abs(beta) * r.abs()
    return v, a


def _ref_fwd_forms(x, w, pad, *, ups, bias, act, slope, chan_scale, alpha, res, beta, in_win, xs, stride, act_c1, act2,
                   mask_y, mask_win, mask_slope):
    """``ref_fwd`` with ``act_c1`` / ``act2`` / a forward-form mask, step by step in the kernel's order"""
    x, w = _win(_d(x), in_win), _d(w)
    if ups:
        x = up2(x)
    v = _conv_slab(x, w, pad, xs, stride)
    a = _conv_slab(x.abs(), w.abs(), pad, xs, stride)
    n = v.shape[1]
    c1 = n if act_c1 is None else min(int(act_c1), n)
    if bias is not None:  # (acc + bias): the bias table holds zeros from act_c1 on
        b = _d(bias).clone().view(1, -1, 1, 1, 1)
        b[:, c1:] = 0.0
        v, a = v + b, a + b.abs()
    r = None if res is None else _d(res)
    if act2:  # the residual joins in front of the activation
        assert r is not None, "act2 needs the partial sums in res"
        v, a = v + beta * r, a + abs(beta) * r.abs()
    if act or act2:
        v = torch.cat([F.leaky_relu(v[:, :c1], slope), v[:, c1:]], dim=1)
    if chan_scale is not None:
        s = _d(chan_scale).view(v.shape[0], n, 1, 1, 1)
        v, a = v * s, a * s.abs()
    v, a = alpha * v, abs(alpha) * a
    if r is not None and not act2:
        v, a = v + beta * r, a + abs(beta) * r.abs()
    if mask_y is not None:
        v, a = _apply_mask(v, a, mask_y, mask_win, mask_slope)
    return v, a


def dgrad_filter(w):
    """(Cout, Cin, KX, KY, KZ) -> the filter of the input gradient as a forward conv over dy: (Cin, Cout, flipped)"""
    return w.transpose(0, 1).flip(2, 3, 4)


def ref_dgrad(gy, w, pad, *, ups=False, alpha=1.0, mask_y=None, slope=0.2, keep=None, acc=None, xs=None, acc_c1=None,
              acc_beta=1.0, mask_win=None):
    """dx = (alpha * conv^T(gy, w) [+ acc]) * lrelu'(mask_y) * keep  for a stride-1 conv with padding ``pad``.
    ``ups``: the conv read up2(x) - dx is then at x's (coarse) resolution, the 2 x 2 fold of the fine gradient;
    ``mask_y`` (B, Cin, ...) the saved output whose sign selects 1 or ``slope``, ``keep`` (B, Cin) the Dropout3d
    channel scale; ``acc`` a value added before the mask (accumulate launches); ``xs`` dx x-planes [x0, x1) only
    (not with ``ups``).

    The halo-tile kernel's epilogue (conv_tile_impl.h :692-713) runs
    ``(acc + bias) -> act -> * (chan_scale * alpha) -> + beta * res -> * mask``, which for the input gradient - no bias,
    no activation, chan_scale = ``keep``, res = the accumulated tensor - is

        dx = (keep * alpha * conv^T(gy, w) + acc_beta * acc[below acc_c1]) * lrelu'(mask_y)[mask window].

    The line at the top multiplies ``keep`` after the mask instead; without ``acc`` that is the same product in another
    order, and every caller from before these forms gets the result it always got, bit for bit.  With any of the
    following given, the reference takes the kernel's order literally:

    * ``acc_c1`` (``accumulate = n``): only produced channels below ``acc_c1`` accumulate;
    * ``acc_beta`` (``wsr_dgrad_opts_t.acc_beta``): the weight of the accumulated value;
    * ``mask_win`` = (c0, c1): the mask covers produced channels [c0, c1) only, ``mask_y`` holding c1 - c0 channels
      (``mask_win=(0, Cin)`` with a whole-width ``mask_y`` is the production form, in the kernel's order).

    ``keep`` with ``acc`` is refused there: the kernel scales the fresh sums only, the generic route (conv_dgrad +
    lrelu_bwd_) scales the accumulated value as well, and no caller combines them.  Returns (ref, A)."""
    gy, w = _d(gy), _d(w)
    k = w.shape[2:]
    tp = tuple(kk - 1 - p for kk, p in zip(k, pad))
    wt = dgrad_filter(w)
    if acc_c1 is not None or acc_beta != 1.0 or mask_win is not None:
        assert keep is None or acc is None, "keep together with an accumulate: the routes disagree, see the docstring"
        v, a = _conv_slab(gy, wt, tp, xs), _conv_slab(gy.abs(), wt.abs(), tp, xs)
        if ups:
            v, a = fold2(v), fold2(a)
        if keep is not None:  # (chan_scale * alpha), one factor per sample and channel
            s = _d(keep).view(v.shape[0], v.shape[1], 1, 1, 1) * alpha
            v, a = v * s, a * s.abs()
        else:
            v, a = alpha * v, abs(alpha) * a
        if acc is not None:
            c1 = v.shape[1] if acc_c1 is None else min(int(acc_c1), v.shape[1])
            r = _d(acc)[:, :c1]
            v, a = v.clone(), a.clone()
            v[:, :c1] += acc_beta * r
            a[:, :c1] += abs(acc_beta) * r.abs()
        if mask_y is not None:
            v, a = _apply_mask(v, a, mask_y, mask_win, slope)
        return v, a
    v = alpha * _conv_slab(gy, wt, tp, xs)
    a = abs(alpha) * _conv_slab(gy.abs(), wt.abs(), tp, xs)
    if ups:
        v, a = fold2(v), fold2(a)
    if acc is not None:
        v, a = v + _d(acc), a + _d(acc).abs()
    if mask_y is not None:
        m = torch.where(_d(mask_y) > 0, 1.0, slope).to(torch.float64)
        v, a = v * m, a * m.abs()
    if keep is not None:
        s = _d(keep).view(v.shape[0], v.shape[1], 1, 1, 1)
        v, a = v * s, a * s.abs()
    return v, a


def ref_wgrad(x, gy, k, pad, *, ups=False, in_win=None):
    """dw[n, c, tap] = sum_{b, v} gy[b, n, v] * up?(x)[b, c, v + tap - pad] (stride 1).  Returns (ref, A) in the master
    layout (Cout, Cin, KX, KY, KZ)."""
    x, gy = _win(_d(x), in_win), _d(gy)
    if ups:
        x = up2(x)
    out = []
    for xx, gg in ((x, gy), (x.abs(), gy.abs())):
        w = torch.zeros((gg.shape[1], xx.shape[1]) + tuple(k), dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv3d(xx, w, None, 1, tuple(pad)), w, gg)
        out.append(g)
    return out[0], out[1]


def _f32(v) -> float:
    """a scalar as the C side receives it (``float`` across the ABI)"""
    return float(torch.tensor(float(v), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm: every stage from the fp32 inputs the kernel itself receives, on (nvox, C) rows and (C,) / (2C,) tables
# ---------------------------------------------------------------------------------------------------------------------

def _row(t):
    return _d(t).reshape(1, -1)


def ref_bn_sums(x, shift=None):
    """{sum_v d, sum_v d^2} per channel as one (2C,) table, d = x - shift[c] (``shift`` None: 0).  Returns (ref, A),
    A = {sum |d|, sum d^2}; bound with K = nvox + rows."""
    d = _d(x) if shift is None else _d(x) - _row(shift)
    return torch.cat([d.sum(0), (d * d).sum(0)]), torch.cat([d.abs().sum(0), (d * d).sum(0)])


def ref_bn_bwd_dy(dy, y, act, slope=0.2):
    """the gradient in front of the folded LeakyReLU, g' = dy * (y > 0 ? 1 : slope) (``act`` false: dy itself), which
    ``bn_bwd_reduce`` writes back over dy.  Returns (g', |g'|); bound with K = 1 and the stored type's rho, and where
    the mask is 1 the stored element is the input, bit for bit."""
    g = _d(dy)
    if act:
        g = g * _lrelu_mask(y, _f32(slope))
    return g, g.abs()


def ref_bn_bwd_sums(dy, y, x, mean, invstd, act, slope=0.2):
    """{sum g', sum g' * xhat} per channel as one (2C,) table, g' of ``ref_bn_bwd_dy`` and xhat = (x - mean) * invstd.
    Returns (ref, A), A = {sum |g'|, sum |g'| |xhat|}; bound with K = nvox + rows."""
    g, _ = ref_bn_bwd_dy(dy, y, act, slope)
    xh = (_d(x) - _row(mean)) * _row(invstd)
    return (torch.cat([g.sum(0), (g * xh).sum(0)]),
            torch.cat([g.abs().sum(0), (g.abs() * xh.abs()).sum(0)]))


def ref_bn_mean(sums, cnt):
    """sums[c] / cnt (``bn_mean``).  Returns (ref, |ref|); bound with K = 1."""
    m = _d(sums) / _f32(cnt)
    return m, m.abs()


def ref_bn_finalize(s1, s2, cnt, mean, eps, momentum, rm0=None, rv0=None):
    """``bn_finalize_channel`` from the shifted sums s1 = sum d, s2 = sum d^2 (d = x - mean): dm = s1 / cnt,
    var = max(s2 / cnt - dm^2, 0), invstd = (var + eps)^-1/2, unb = var * cnt / max(cnt - 1, 1) and the running
    statistics rm = (1 - m) rm0 + m mean, rv = (1 - m) rv0 + m unb (absent without rm0 / rv0).  Returns (ref, A), two
    dicts: ref of ``var, invstd, unb, rm, rv``; A of ``var`` (= s2 / cnt + dm^2), ``rm`` and ``rv`` (the two terms'
    magnitudes, rv's with A_var for var).  ``bn_finalize_bounds`` turns them into bounds."""
    s1, s2, mean = _d(s1), _d(s2), _d(mean)
    cnt, eps, m = _f32(cnt), _f32(eps), _f32(momentum)
    dm = s1 / cnt
    var = (s2 / cnt - dm * dm).clamp_min(0.0)
    a_var = s2.abs() / cnt + dm * dm
    ub = cnt / max(cnt - 1.0, 1.0)
    ref = {"var": var, "invstd": (var + eps) ** -0.5, "unb": var * ub}
    A = {"var": a_var}
    if rm0 is not None:
        rm0, rv0 = _d(rm0), _d(rv0)
        ref["rm"] = (1.0 - m) * rm0 + m * mean
        ref["rv"] = (1.0 - m) * rv0 + m * ref["unb"]
        A["rm"] = abs(1.0 - m) * rm0.abs() + abs(m) * mean.abs()
        A["rv"] = abs(1.0 - m) * rv0.abs() + abs(m) * a_var * ub
    return ref, A


def bn_finalize_bounds(ref, A, eps, steps=1):
    """bounds of ``invstd``, ``rm``, ``rv`` from ``ref_bn_finalize`` / ``ref_bn_running`` with the same ``eps``
    (``steps`` = G for running statistics after G ordered updates: K = 3G and 5G)"""
    vb = bound(ref["var"], A["var"], 3, 0.0)
    out = {"invstd": ref["invstd"] * (0.5 * vb / (ref["var"] + _f32(eps)) + LAMBDA * U_FP32)}
    if "rm" in ref:
        out["rm"] = bound(ref["rm"], A["rm"], 3 * steps, 0.0)
        out["rv"] = bound(ref["rv"], A["rv"], 5 * steps, 0.0)
    return out


def ref_bn_running(groups, cnt, eps, momentum, rm0, rv0):
    """the running statistics after ``ref_bn_finalize`` of each (s1, s2, mean) of ``groups`` in order, in float64 from
    the fp32 initial values.  Returns (ref, A, per-group finalize results): A the running sum of term magnitudes.
    Bound with ``steps=len(groups)``."""
    rm, rv = _d(rm0), _d(rv0)
    a_rm, a_rv = rm.abs(), rv.abs()
    m = _f32(momentum)
    cntf = _f32(cnt)
    ub = cntf / max(cntf - 1.0, 1.0)
    per = []
    for s1, s2, mean in groups:
        r, a = ref_bn_finalize(s1, s2, cnt, mean, eps, momentum, rm, rv)
        a_rm = abs(1.0 - m) * a_rm + abs(m) * _d(mean).abs()
        a_rv = abs(1.0 - m) * a_rv + abs(m) * a["var"] * ub
        rm, rv = r["rm"], r["rv"]
        per.append((r, a))
    last = per[-1][0]
    ref = {"rm": rm, "rv": rv, "var": last["var"], "invstd": last["invstd"]}
    return ref, {"rm": a_rm, "rv": a_rv, "var": per[-1][1]["var"]}, per


def bn_v4_geometry(C, nvox):
    """(lanes, rows) of ``bn_reduce_v4_kernel`` as ``bn_v4_grid`` (elementwise.hip) launches it: lanes = 256 / (C / 4),
    rows = min(512, ceil(nvox / (16 lanes))).  Widths the vectorised kernels do not take (C % 4, C > 512) go to the
    scalar atomic kernels: lanes is None and rows the workgroup count of ``bn_grid``."""
    if C % 4 or C > 512:
        return None, max(1, min(1024, -(-nvox * C // (256 * 64))))
    lanes = 256 // (C // 4)
    return lanes, max(1, min(512, -(-nvox // (16 * lanes))))


def ref_bn_apply(x, mean, invstd, gamma, beta, act, slope=0.2):
    """y = lrelu?((x - mean) * invstd * gamma + beta).  Returns (ref, A), A = |x - mean| invstd |gamma| + |beta|;
    bound with K = 4 and the stored type's rho."""
    d = _d(x) - _row(mean)
    sc = _row(invstd) * _row(gamma)
    v = d * sc + _row(beta)
    a = d.abs() * sc.abs() + _row(beta).abs()
    if act:
        v = F.leaky_relu(v, _f32(slope))
    return v, a


def ref_bn_bwd_apply(g, x, act_y, slope, mean, invstd, gamma, sums, inv_n):
    """dx = (g' - sums[c] inv_n - xhat sums[C + c] inv_n) * gamma * invstd with g' = g * (act_y > 0 ? 1 : slope)
    (``act_y`` None: g) and xhat = (x - mean) * invstd; both mean terms are absent when ``sums`` is None (the
    eval-mode pass).  Returns (ref, A), A the three terms' magnitudes times |gamma invstd|; bound with K = 8 and the
    stored type's rho - the one-element kernel and the 8-wide one, which orders the products differently."""
    v = _d(g)
    if act_y is not None:
        v = v * _lrelu_mask(act_y, _f32(slope))
    a = v.abs()
    if sums is not None:
        s, n = _d(sums), _f32(inv_n)
        C = v.shape[1]
        xh = (_d(x) - _row(mean)) * _row(invstd)
        t1, t2 = s[:C].reshape(1, -1) * n, xh * s[C:].reshape(1, -1) * n
        v, a = v - t1 - t2, a + t1.abs() + t2.abs()
    sc = _row(gamma) * _row(invstd)
    return v * sc, a * sc.abs()


def ref_pointwise(x, w, *, bias=None, act=False, slope=0.2, alpha=1.0, res=None, beta=0.0, res_c1=None, res2=None,
                  beta2=0.0, mask_y=None, mask_win=None, mask_slope=0.2):
    """y = alpha * lrelu?(x @ w.T + bias) + beta * res[:, :c1] + beta2 * res2[:, :c1] on logical matrices: x (nvox, red),
    w (n_out, red), the residuals (nvox, >= c1) with c1 = ``res_c1`` (default n_out; zero past it).  Columns
    ``mask_win`` = [c0, c1) of y are then multiplied by 1 where ``mask_y`` (nvox, c1 - c0) > 0, else by ``mask_slope``.
    The scalars are taken as the fp32 values the C side receives.  For the input gradient pass x = dy and w = W.T.
    Returns (ref, A)."""
    x, w = _d(x), _d(w)
    alpha, beta, beta2, slope, mask_slope = (_f32(s) for s in (alpha, beta, beta2, slope, mask_slope))
    v, a = x @ w.T, x.abs() @ w.abs().T
    if bias is not None:
        b = _d(bias).view(1, -1)
        v, a = v + b, a + b.abs()
    if act:
        v = F.leaky_relu(v, slope)
    v, a = alpha * v, abs(alpha) * a
    c1 = v.shape[1] if res_c1 is None else min(res_c1, v.shape[1])
    for r, s in ((res, beta), (res2, beta2)):
        if r is not None:
            r = _d(r)[:, :c1]
            v[:, :c1] += s * r
            a[:, :c1] += abs(s) * r.abs()
    if mask_y is not None:
        m0, m1 = mask_win
        m = torch.where(_d(mask_y) > 0, 1.0, mask_slope).to(torch.float64)
        assert m.shape == (v.shape[0], m1 - m0), (tuple(m.shape), mask_win)
        v[:, m0:m1] *= m
        a[:, m0:m1] *= m.abs()
    return v, a


# ---------------------------------------------------------------------------------------------------------------------
# the network boundary: derivative stencils, the content loss, the planar layout kernels (test_boundary_matrix.py)
# ---------------------------------------------------------------------------------------------------------------------

K_STENCIL = 12   # one derivative element, see the module docstring
K_ADJOINT = 19   # one element of the stencils' adjoint
K_RESIDUAL = 23  # one element of the content loss's residual
K_DSR = 24       # one element of d loss / d SR
PL_BLOCK, PL_ROWS = 256, 1024  # physics_loss.hip :25-26


def physics_rows(nvox) -> int:
    """workgroups of ``physics_stats_kernel`` = partial rows of its final kernel (``pl_grid``, physics_loss.hip :223)"""
    return max(1, min(PL_ROWS, -(-int(nvox) // PL_BLOCK)))


def _stencil_rows(co):
    """rows of the derivative operator along the LAST axis of the float64 coordinates ``co`` (..., n), as
    ``deriv_row`` (stencil.h) builds them: (a, b, c, bmag), bmag the centre weight's magnitude BEFORE the cancellation
    in hr^2 - hl^2.  n < 2: zeros."""
    n = co.shape[-1]
    a, b, c, bm = (torch.zeros_like(co) for _ in range(4))
    if n < 2:
        return a, b, c, bm
    h = co[..., 1:] - co[..., :-1]
    if n >= 3:
        hl, hr = h[..., :-1], h[..., 1:]
        den = hl * hr * (hl + hr)
        a[..., 1:-1] = -(hr * hr) / den
        b[..., 1:-1] = (hr * hr - hl * hl) / den
        c[..., 1:-1] = (hl * hl) / den
        bm[..., 1:-1] = (hr * hr + hl * hl) / den.abs()
    b[..., 0], c[..., 0] = -1.0 / h[..., 0], 1.0 / h[..., 0]
    a[..., -1], b[..., -1] = -1.0 / h[..., -1], 1.0 / h[..., -1]
    bm[..., 0], bm[..., -1] = b[..., 0].abs(), b[..., -1].abs()
    return a, b, c, bm


def _shift(t, k):
    """s[..., i] = t[..., i + k], zero where i + k falls outside"""
    s = torch.zeros_like(t)
    n = t.shape[-1]
    if abs(k) < n:
        if k > 0:
            s[..., :n - k] = t[..., k:]
        else:
            s[..., -k:] = t[..., :n + k]
    return s


def _axis_coords(co, dim):
    co = _d(co)
    return co if co.dim() == 1 else co.movedim(dim, -1)


def ref_deriv(f, co, dim):
    """derivative of f (B, C, X, Y, Z) along ``dim``: three-point non-uniform rows inside, one-sided rows at the ends,
    zero on an axis of length 1.  ``co``: a 1-D table of the axis (x, y) or a field (B, 1, X, Y, Z) whose columns
    along ``dim`` are the coordinates (z).  Returns (d, M), M = |a| |f-| + bmag |f0| + |c| |f+| with bmag taken before
    the cancellation of the centre weight; bound with K_STENCIL."""
    f = _d(f).movedim(dim, -1)
    a, b, c, bm = _stencil_rows(_axis_coords(co, dim))
    fm, fp = _shift(f, -1), _shift(f, 1)
    v = a * fm + b * f + c * fp
    m = a.abs() * fm.abs() + bm * f.abs() + c.abs() * fp.abs()
    return v.movedim(-1, dim), m.movedim(-1, dim)


def ref_wind_gradient(f, x, y, zc):
    """the 9-channel Jacobian stack (B, 9, X, Y, Z) of f (B, 3, X, Y, Z): d/dx, d/dy, d/dz of the three components, z
    on the per-column heights ``zc`` (B, 1, X, Y, Z).  Returns (J, M); bound with K_STENCIL."""
    parts = [ref_deriv(f, x, 2), ref_deriv(f, y, 3), ref_deriv(f, zc, 4)]
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)


def _adjoint_axis(g, co, dim):
    g = g.movedim(dim, -1)
    a, b, c, bm = _stencil_rows(_axis_coords(co, dim))
    v = _shift(c * g, -1) + b * g + _shift(a * g, 1)
    m = _shift(c.abs() * g.abs(), -1) + bm * g.abs() + _shift(a.abs() * g.abs(), 1)
    return v.movedim(-1, dim), m.movedim(-1, dim)


def ref_wind_gradient_bwd(g, x, y, zc):
    """adjoint of ``ref_wind_gradient``: df_j = c_{j-1} g_{j-1} + b_j g_j + a_{j+1} g_{j+1} along each axis, summed
    over the three axes; g (B, 9, X, Y, Z) -> (B, 3, X, Y, Z).  Returns (df, A), A the same expression on magnitudes
    with the pre-cancellation centre weight; bound with K_ADJOINT."""
    g = _d(g)
    parts = [_adjoint_axis(g[:, 3 * k:3 * k + 3], co, 2 + k) for k, co in enumerate((x, y, zc))]
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def _nanmax(t):
    return t.max()  # (torch.max propagates NaN)


def ref_physics_stats(hr, sr, x, y, zc, rows=None, jac=None, tight_sums=False):
    """the 14 statistics of ``wsr_physics_loss_stats``: sums {xy Jacobian, z Jacobian, div3, div2 squared differences,
    sum |HR - SR|, sum (HR - SR)^2}, then the maxima {max |J[:6]|, max J[6:] (signed), max |div3|, max |div2|} of HR
    and of SR.  Returns (ref, bnd), two (14,) tensors.  Sums: ``bound(ref, A, K, 0)`` with A = sum (M_sr + M_hr)^2
    (the pixel sums: sum |d|, sum d^2) and K = terms + rows + the per-term roundings of the module docstring,
    ``rows`` = ``physics_rows(voxels)``.  Maxima: the largest per-element bound over the elements the maximum ranges
    over (max is 1-Lipschitz), rho = 0.  A NaN anywhere in a range makes that entry NaN.

    ``tight_sums``: a third (6,) tensor, a second and narrower bound of the sums.  Where SR is close to HR on fields
    with a large mean, (M_sr + M_hr)^2 is 10^4 times the term (J_sr - J_hr)^2 and the bound above several times the sum
    itself.  The narrower one follows the error through the square: each Jacobian entry is within its own element
    bound e_sr, e_hr (K_STENCIL; + 2, + 1 for the divergences), so a term is off by at most 2 |d| e + e^2 with
    e = e_sr + e_hr, summed without any cancellation, plus ``bound(s, s, terms + rows + 2, 0)`` for the difference,
    the square and the additions of the terms themselves.  The pixel sums keep their bound."""
    hr_, sr_ = _d(hr), _d(sr)
    nvox = hr_.numel() // 3
    rows = physics_rows(nvox) if rows is None else rows
    (jh, mh), (js, ms) = jac if jac is not None else (ref_wind_gradient(hr, x, y, zc), ref_wind_gradient(sr, x, y, zc))
    d3 = lambda j: j[:, 0] + j[:, 4] + j[:, 8]  # noqa: E731
    d2 = lambda j: j[:, 0] + j[:, 4]  # noqa: E731
    d = hr_ - sr_
    ref, bnd, tight = [], [], []
    eb = lambda j, m, k: bound(j, m, k, 0.0)  # noqa: E731
    for val, a, terms, per, e in (
            ((js[:, :6] - jh[:, :6]) ** 2, (ms[:, :6] + mh[:, :6]) ** 2, 6, 27,
             eb(js[:, :6], ms[:, :6], K_STENCIL) + eb(jh[:, :6], mh[:, :6], K_STENCIL)),
            ((js[:, 6:] - jh[:, 6:]) ** 2, (ms[:, 6:] + mh[:, 6:]) ** 2, 3, 27,
             eb(js[:, 6:], ms[:, 6:], K_STENCIL) + eb(jh[:, 6:], mh[:, 6:], K_STENCIL)),
            ((d3(jh) - d3(js)) ** 2, (d3(mh) + d3(ms)) ** 2, 1, 31,
             eb(d3(js), d3(ms), K_STENCIL + 2) + eb(d3(jh), d3(mh), K_STENCIL + 2)),
            ((d2(jh) - d2(js)) ** 2, (d2(mh) + d2(ms)) ** 2, 1, 29,
             eb(d2(js), d2(ms), K_STENCIL + 1) + eb(d2(jh), d2(mh), K_STENCIL + 1)),
            (d.abs(), d.abs(), 3, 1, None), (d * d, d * d, 3, 3, None)):
        s = val.sum()
        ref.append(s)
        bnd.append(bound(s, a.sum(), terms * nvox + rows + per, 0.0))
        if e is not None:  # a term (d + t)^2 with |t| <= e is off by at most 2 |d| e + e^2; then the sum of the terms
            tight.append((2.0 * val.sqrt() * e + e * e).sum() + bound(s, s, terms * nvox + rows + 2, 0.0))
        else:
            tight.append(bnd[-1])
    for j, m in ((jh, mh), (js, ms)):
        for val, b in ((j[:, :6].abs(), bound(j[:, :6], m[:, :6], K_STENCIL, 0.0)),
                       (j[:, 6:], bound(j[:, 6:], m[:, 6:], K_STENCIL, 0.0)),
                       (d3(j).abs(), bound(d3(j), d3(m), K_STENCIL + 2, 0.0)),
                       (d2(j).abs(), bound(d2(j), d2(m), K_STENCIL + 1, 0.0))):
            ref.append(_nanmax(val))
            fin = b[torch.isfinite(b)]
            bnd.append(fin.max() if fin.numel() else torch.tensor(TINY, dtype=torch.float64))
    if tight_sums:
        return torch.stack(ref), torch.stack(bnd), torch.stack(tight)
    return torch.stack(ref), torch.stack(bnd)


def ref_physics_residual(hr, sr, x, y, zc, coef, jac=None):
    """the first launch of ``wsr_physics_loss_bwd``: r[k] = 2 coef_g (J_sr[k] - J_hr[k]) with g = 0 for k < 6, 1 for
    k >= 6, plus 2 coef_2 (div3_sr - div3_hr) on channels 0, 4, 8 and 2 coef_3 (div2_sr - div2_hr) on channels 0, 4
    (physics_loss.hip :160-167).  A coefficient that is exactly zero drops its term, whatever the Jacobians hold.
    ``jac``: ((J_hr, M_hr), (J_sr, M_sr)) of ``ref_wind_gradient`` where the caller has them already.
    Returns (r, A); bound with K_RESIDUAL."""
    cf = [2.0 * float(v) for v in _d(coef)[:4]]
    (jh, mh), (js, ms) = jac if jac is not None else (ref_wind_gradient(hr, x, y, zc), ref_wind_gradient(sr, x, y, zc))
    r, a = torch.zeros_like(js), torch.zeros_like(js)
    for g, sl in ((cf[0], slice(0, 6)), (cf[1], slice(6, 9))):
        if g != 0.0:
            r[:, sl] = g * (js[:, sl] - jh[:, sl])
            a[:, sl] = abs(g) * (ms[:, sl] + mh[:, sl])
    for g, chans in ((cf[2], (0, 4, 8)), (cf[3], (0, 4))):
        if g != 0.0:
            t = g * sum(js[:, k] - jh[:, k] for k in chans)
            ta = abs(g) * sum(ms[:, k] + mh[:, k] for k in chans)
            for k in chans:
                r[:, k] += t
                a[:, k] += ta
    return r, a


def ref_physics_adjoint(res, hr, sr, x, y, zc, coef):
    """the second launch: dsr = adjoint of the stencils applied to ``res`` (skipped altogether when coef[0..3] are all
    zero: 1 / dz of two equal levels must not meet the zeros) + coef[4] sign(d) + 2 coef[5] d, d = SR - HR, each pixel
    term only where its coefficient is not zero.  Returns (dsr, A); bound with K_DSR."""
    cf = [float(v) for v in _d(coef)]
    d = _d(sr) - _d(hr)
    if any(v != 0.0 for v in cf[:4]):
        v, a = ref_wind_gradient_bwd(res, x, y, zc)
    else:
        v, a = torch.zeros_like(d), torch.zeros_like(d)
    if cf[4] != 0.0:
        v, a = v + cf[4] * torch.sign(d), a + abs(cf[4]) * torch.sign(d).abs()
    if cf[5] != 0.0:
        v, a = v + 2.0 * cf[5] * d, a + 2.0 * abs(cf[5]) * d.abs()
    return v, a


def ref_physics_bwd(hr, sr, x, y, zc, coef, residual=None, jac=None):
    """``wsr_physics_loss_bwd``: ((residual, A), (dsr, A)).  ``residual``: the fp32 buffer the first launch wrote - dsr is
    then referenced from it, as the BatchNorm stages are from their predecessor's tables - else the float64 one."""
    r = ref_physics_residual(hr, sr, x, y, zc, coef, jac)
    return r, ref_physics_adjoint(r[0] if residual is None else residual, hr, sr, x, y, zc, coef)


def ref_zfold(t, bias, C, KZ, pz):
    """y[b, c, ..., z] = bias[c] + sum_k t[b, c KZ + k, ..., z + k - pz] (taps outside [0, Z) absent); t (B, C KZ, ...,
    Z).  Returns (y, A), A = |bias| + sum |t|; bound with K = KZ + 1."""
    t = _d(t)
    B, Z = t.shape[0], t.shape[-1]
    t = t.reshape((B, C, KZ) + tuple(t.shape[2:]))
    v = torch.zeros((B, C) + tuple(t.shape[3:]), dtype=torch.float64)
    a = torch.zeros_like(v)
    if bias is not None:
        b = _d(bias).view((1, C) + (1,) * (v.dim() - 2))
        v, a = v + b, a + b.abs()
    for k in range(KZ):
        s = _shift(t[:, :, k], k - pz)
        v, a = v + s, a + s.abs()
    return v, a


def ref_zunfold(g, KZ, pz, c_fill):
    """the adjoint of the fold as a copy: d[b, ..., z, c KZ + k] = g[b, c, ..., z - k + pz] or 0, channels from C KZ to
    ``c_fill`` zero; g planar fp32 (B, C, X, Y, Z) -> fp32 (B, X, Y, Z, c_fill), every element a bit pattern of g or
    +0.0 (no arithmetic: compared as bits)."""
    B, C = g.shape[:2]
    gi = g.detach().cpu().contiguous().view(torch.int32)
    oi = torch.zeros((B,) + tuple(g.shape[2:]) + (c_fill,), dtype=torch.int32)
    for c in range(C):
        for k in range(KZ):
            oi[..., c * KZ + k] = _shift(gi[:, c], pz - k)
    return oi.view(torch.float32)


def boundary_inputs(shape, coords="random", seed=0, descending=False):
    """fp32 CPU operands (hr, sr, x, y, zc) of the content loss at ``shape`` = (B, X, Y, Z).  ``coords``: "random"
    (non-uniform, spacings 50-150 in x and y, 6-36 in z), "uniform" (exactly), "near" (100 i + 1e-5 i^1.5: the centre
    weight cancels almost completely; "near_odd": 100.37 i + 1e-5 i^1.5, whose spacings have low bits set, so that
    their squares round) or "heights" (x, y random; columns start near 1000 m with spacings of 5-50 m
    that vary per column, like the data's terrain-following levels).  The heights always differ between samples.
    Fields: 10 + randn, SR = HR + 0.1 randn (the stencil cancels a mean of 10); ``descending``: both fall by about 2
    per level, every z-derivative negative."""
    B, X, Y, Z = shape
    gen = torch.Generator().manual_seed(seed)
    f64 = torch.float64

    def axis(n, kind, step=100.0):
        i = torch.arange(n, dtype=f64)
        if kind == "uniform":
            return 100.0 * i
        if kind == "near":
            return step * i + 1e-5 * i ** 1.5
        return torch.cumsum(torch.rand(n, generator=gen, dtype=f64) + 0.5, 0) * 100.0

    kind = coords if coords in ("uniform", "near") else "random"
    if coords == "near_odd":
        kind = "near"
    step = 100.37 if coords == "near_odd" else 100.0
    x, y = axis(X, kind, step), axis(Y, kind, step)
    scale = (1.0 + torch.arange(B, dtype=f64)).view(B, 1, 1, 1, 1)
    if coords == "uniform":
        zc = (30.0 * torch.arange(Z, dtype=f64)).expand(B, 1, X, Y, Z) * scale
    elif kind == "near":
        zc = axis(Z, "near", step).expand(B, 1, X, Y, Z) * (0.5 + 0.5 * scale)
    elif coords == "heights":
        dz = 5.0 + 45.0 * torch.rand((B, 1, X, Y, Z), generator=gen, dtype=f64)
        zc = 1000.0 + 50.0 * torch.rand((B, 1, X, Y, 1), generator=gen, dtype=f64) + torch.cumsum(dz, -1)
    else:
        zc = torch.cumsum(torch.rand((B, 1, X, Y, Z), generator=gen, dtype=f64) + 0.2, -1) * 30.0
    hr = 10.0 + torch.randn((B, 3, X, Y, Z), generator=gen, dtype=f64)
    if descending:
        hr = 10.0 - 2.0 * torch.arange(Z, dtype=f64) + 0.1 * torch.randn((B, 3, X, Y, Z), generator=gen, dtype=f64)
    sr = hr + (0.05 if descending else 0.1) * torch.randn((B, 3, X, Y, Z), generator=gen, dtype=f64)
    return tuple(t.float().contiguous() for t in (hr, sr, x, y, zc))


# ---------------------------------------------------------------------------------------------------------------------
# the table Adam family (test_optimizer_matrix.py)
# ---------------------------------------------------------------------------------------------------------------------

ADAM_CHUNK = 32768        # elements per job of the table (hip_ops.ADAM_CHUNK)
K_ADAM_M, K_ADAM_V, K_ADAM_P = 5, 6, 3
K_CLIP_G = 3              # the written-back gradient coef * g


def adam_hyper(lr, betas, eps, wd, step, f32_hyper=False):
    """the eight factors of one Adam step in float64 - (beta1, 1 - beta1, beta2, 1 - beta2, step_size = lr / bc1,
    sqrt(bc2), eps, wd) - from Python doubles, as ``torch.optim.Adam`` holds them.  ``f32_hyper``: from the fp32 values
    the single-tensor entry ``wsr_adam_step`` receives across its ABI (then 1 - float(beta) is exact in fp32 for beta
    in [0.5, 1], and the kernel's ``1.f - beta`` equals it)."""
    b1, b2 = betas
    if f32_hyper:
        lr, b1, b2, eps, wd = (_f32(s) for s in (lr, b1, b2, eps, wd))
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    return b1, 1.0 - b1, b2, 1.0 - b2, lr / bc1, math.sqrt(bc2), float(eps), float(wd)


def ref_adam(p, g, m, v, lr, betas, eps, wd, step, coef=None, *, f32_hyper=False):
    """one step of ``torch.optim.Adam`` (L2 weight decay, both bias corrections, eps outside the square root) in float64
    from the fp32 tensors the kernel receives; ``coef``: the clip coefficient, the gradient is coef * g.
    Returns ((p', bound), (m', bound), (v', bound)), the bounds propagated as the module docstring derives them."""
    b1, omb1, b2, omb2, ss, bc2s, eps, wd = adam_hyper(lr, betas, eps, wd, step, f32_hyper)
    p, g, m, v = (_d(t) for t in (p, g, m, v))
    km, kv = K_ADAM_M, K_ADAM_V
    if coef is not None:  # three roundings into coef * g (K_CLIP_G), once in m', twice in v'
        g = float(coef) * g
        km, kv = km + K_CLIP_G, kv + 2 * K_CLIP_G
    ge = g + wd * p
    ga = g.abs() + wd * p.abs()
    m1 = b1 * m + omb1 * ge
    v1 = b2 * v + omb2 * ge * ge
    a_m = b1 * m.abs() + omb1 * ga
    a_v = b2 * v.abs() + omb2 * ga * ga
    bm, bv = bound(m1, a_m, km, 0.0), bound(v1, a_v, kv, 0.0)
    s = v1.clamp_min(0.0).sqrt()
    # |sqrt(v' + e) - sqrt(v')| for |e| <= bv, exactly: bv / (2 sqrt v') to first order, sqrt(bv) at v' = 0
    bs = torch.maximum((v1.clamp_min(0.0) + bv).sqrt() - s, s - (v1 - bv).clamp_min(0.0).sqrt())
    den = s / bc2s + eps
    bden = bs / bc2s + LAMBDA * math.sqrt(3.0) * U_FP32 * den
    q_mag = a_m / den
    lo = (den - bden).clamp_min(TINY)
    bq = (bm + q_mag * bden) / lo + LAMBDA * U_FP32 * q_mag
    p1 = p - ss * (m1 / den)
    bp = abs(ss) * bq + bound(p1, p.abs() + abs(ss) * q_mag, K_ADAM_P, 0.0)
    return (p1, bp), (m1, bm), (v1, bv)


def adam_case(n, step, seed, plant=True):
    """fp32 CPU (p, g, m, v) of one tensor of n elements: p, g = randn; state zero at step 1, else m = 0.3 randn,
    v = (0.5 randn)^2.  ``plant``: the designed elements at 0, 4 (n >> 2) (the first tail element), n - 1 and the first
    and last element of a second chunk, in turn (starting with ``seed`` % 4): g = m = v = 0; g = 0, v = 0, m = 0.25;
    g = +-1e-25 with v = 0; g = 1e15."""
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = 0.3 * torch.randn(n, generator=gen), (0.5 * torch.randn(n, generator=gen)) ** 2
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    if plant:
        pos = sorted({i for i in (0, 4 * (n >> 2), n - 1, ADAM_CHUNK, 2 * ADAM_CHUNK - 1) if 0 <= i < n})
        for j, i in enumerate(pos):
            kind = (j + seed) % 4
            if kind == 0:
                g[i], m[i], v[i] = 0.0, 0.0, 0.0
            elif kind == 1:
                g[i], v[i], m[i] = 0.0, 0.0, 0.25
            elif kind == 2:
                g[i], v[i] = (1e-25 if j % 2 else -1e-25), 0.0
            else:
                g[i] = 1e15
    return p, g, m, v


def adam_jobs(sizes):
    """[(tensor index, first element, elements)] of the job table ``hip_ops.adam_job_table`` builds for tensors of
    ``sizes`` elements: chunks of ``ADAM_CHUNK``"""
    return [(i, off, min(ADAM_CHUNK, n - off)) for i, n in enumerate(sizes) for off in range(0, n, ADAM_CHUNK)]


def ref_grad_sqnorm(g):
    """sum of g^2 of one job's chunk in float64.  Returns (ref, bound) with K = n + 10 - n squares and additions over
    the 4 accumulators of a thread, its (a0 + a1) + (a2 + a3), six butterfly steps and the four wave sums - rho = 0,
    A = the sum itself (every term is non-negative)."""
    g = _d(g)
    s = (g * g).sum()
    return s, bound(s, s, g.numel() + 10, 0.0)


def ref_clip_total(partials):
    """sqrt of the sum of the fp32 partials in float64 (the kernel adds them in double and rounds the root once).
    Returns (ref, bound) with K = n_jobs + 2, A = the root."""
    t = _d(partials).sum().sqrt()
    return t, bound(t, t, partials.numel() + 2, 0.0)


def clip_coef(total, max_norm):
    """min(1, max_norm / (total + 1e-6)) in float64 from the fp32 ``total`` the kernel wrote and the fp32 ``max_norm``
    and 1e-6 it computes with; NaN stays NaN, as ``c > 1 ? 1 : c`` leaves it.  1.0 for an infinite bound (measure
    only)."""
    if math.isinf(max_norm):
        return 1.0
    c = _f32(max_norm) / (float(total) + _f32(1e-6))
    return 1.0 if c > 1.0 else c


def ema_step_bound(d, e_old, p_new):
    """the shadow's bound of test_ema.py (``step_bound``): 3 u (|d e| + |(1 - d) p|)"""
    return 3 * U_FP32 * ((d * _d(e_old)).abs() + ((1.0 - d) * _d(p_new)).abs())


# ---------------------------------------------------------------------------------------------------------------------
# the activation-gradient and bias-gradient glue (test_glue_matrix.py)
# ---------------------------------------------------------------------------------------------------------------------

def ref_lrelu_bwd(g, y, slope, chan_scale=None, vox_per_b=None):
    """g * (y > 0 ? 1 : slope) * chan_scale[b, c] on window rows (nvox, C); sample b = voxel // vox_per_b.
    Returns (ref, |ref|, factor); bound with K = 2 (slope * scale, then the product with g) and the stored type's rho;
    where ``factor`` is exactly 1 the stored element is the input, bit for bit."""
    f = _lrelu_mask(y, _f32(slope))
    if chan_scale is not None:
        nvox = f.shape[0]
        b = torch.arange(nvox) // int(vox_per_b)
        f = f * _d(chan_scale)[b]
    r = _d(g) * f
    return r, r.abs(), f


def ref_chan_axpby(src, dst, alpha, beta):
    """alpha * src + beta * dst (``dst`` not read when beta == 0).  Returns (ref, A); K = 3, rho once."""
    al, be = _f32(alpha), _f32(beta)
    s = _d(src)
    v, a = al * s, abs(al) * s.abs()
    if be != 0.0:
        d = _d(dst)
        v, a = v + be * d, a + abs(be) * d.abs()
    return v, a


def ref_upsample2_bwd(dy):
    """the 2 x 2 sum in x and y of an NDHWC gradient (B, 2 Xi, 2 Yi, Zi, C) -> (B, Xi, Yi, Zi, C).  Returns (ref, A);
    K = 3 (three additions), A = the sum of the four magnitudes."""
    d = _d(dy)
    B, X2, Y2, Z, C = d.shape
    r = d.reshape(B, X2 // 2, 2, Y2 // 2, 2, Z, C)
    return r.sum(dim=(2, 4)), r.abs().sum(dim=(2, 4))


def chan_sum_geometry(C, nvox, max_rows=512):
    """(groups, lanes, rows) of ``chan_sum_kernel`` as ``wsr_chan_sum`` launches it: 4-channel groups, voxel lanes per
    workgroup 256 / groups, rows = min(512, ceil(nvox / (16 lanes))) workgroups = partial rows"""
    groups = C // 4
    lanes = 256 // groups
    return groups, lanes, max(1, min(max_rows, -(-nvox // (16 * lanes))))


def ref_chan_sum(x, scale=1.0):
    """scale * sum over voxels of window rows (nvox, C).  Returns (ref, A), A = |scale| sum |x|; K = nvox + rows."""
    x, sc = _d(x), _f32(scale)
    return sc * x.sum(0), abs(sc) * x.abs().sum(0)


def ref_chan_sum_partials(x, C, nvox):
    """the partial table (rows, C) of ``chan_sum_kernel``: row r sums the voxels v with (v // lanes) % rows == r.
    Returns (ref, A); a row holds at most ceil(nvox / rows) terms and ``lanes`` lane sums: K = that + lanes."""
    _, lanes, rows = chan_sum_geometry(C, nvox)
    x = _d(x)
    r = (torch.arange(nvox) // lanes) % rows
    ref = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, r, x)
    return ref, torch.zeros(rows, C, dtype=torch.float64).index_add_(0, r, x.abs())


def plane_sum_rows(B, V, max_rows=512) -> tuple:
    """(rv, bper, rows) of ``wsr_plane_sum`` (elementwise.hip :1783-1791): rv voxel slices per batch group of bper
    samples, rows = rv * groups partial rows"""
    rv = max(1, min(max_rows, (V + 16383) // 16384))
    groups = max(1, min(B, max_rows // rv))
    bper = -(-B // groups)
    groups = -(-B // bper)
    return rv, bper, rv * groups


def ref_plane_sum(src):
    """out[c] = sum over samples and voxels of a planar (B, C, ...) tensor.  Returns (ref, A), A the sum of magnitudes;
    bound with K = B V + rows."""
    s = _d(src)
    s = s.reshape(s.shape[0], s.shape[1], -1)
    return s.sum((0, 2)), s.abs().sum((0, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the bound and its check
# ---------------------------------------------------------------------------------------------------------------------

def bound(ref, A, K, rho, rho_mag=None):
    """rho * |ref| + LAMBDA * sqrt(K) * 2^-24 * A + 2^-100 (``rho_mag`` replaces |ref| when several stored values
    were rounded: the sum of their magnitudes)"""
    mag = ref.abs() if rho_mag is None else rho_mag
    return rho * mag + LAMBDA * math.sqrt(K) * U_FP32 * A + TINY


#: worst |err| / bound seen per label (up to its first "[") in this process: the calibration table of a test log
WORST: dict = {}


def _coords(idx, shape, kind):
    c = []
    for s in reversed(shape):
        c.append(idx % s)
        idx //= s
    c = tuple(reversed(c))
    if kind == "filter":  # (n, c, kx, ky, kz) -> (n, tap, c)
        n, ci, kx, ky, kz = c
        return f"(n={n}, tap={(kx * shape[3] + ky) * shape[4] + kz}, c={ci})"
    return "(b={}, c={}, x={}, y={}, z={})".format(*c) if len(c) == 5 else str(c)


def check_within(got, ref, bnd):
    """(number of violations, worst |err| / bound, flat indices of the worst elements, ratio tensor); a non-finite
    element of ``got`` counts as an infinite ratio"""
    got = got.detach().to(torch.float64).cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(got), err / bnd, torch.full_like(err, math.inf))
    flat = ratio.flatten()
    bad = int((flat > 1.0).sum())
    worst = float(flat.max()) if flat.numel() else 0.0
    top = torch.topk(flat, min(5, flat.numel())).indices.tolist() if flat.numel() else []
    return bad, worst, top, ratio


def assert_within(got, ref, bnd, label, kind="act"):
    """every element of ``got`` within ``bnd`` of ``ref``; the message names the violating elements' coordinates
    ((b, c, x, y, z) of activations, (n, tap, c) of filter gradients ``kind="filter"``).  Returns the worst ratio."""
    bad, worst, top, ratio = check_within(got, ref, bnd)
    key = label.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if bad:
        flat_g = got.detach().to(torch.float64).cpu().flatten()
        flat_r, flat_b, flat_q = ref.flatten(), bnd.flatten(), ratio.flatten()
        lines = [f"  {_coords(i, tuple(ref.shape), kind)}: got {float(flat_g[i]):.9g} ref {float(flat_r[i]):.9g} "
                 f"bound {float(flat_b[i]):.3g} ratio {float(flat_q[i]):.3g}" for i in top]
        raise AssertionError(f"{label}: {bad} of {ref.numel()} elements outside the bound, worst |err|/bound "
                             f"{worst:.3g}; worst elements:\n" + "\n".join(lines))
    print(f"[bound] {label}: worst |err|/bound {worst:.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------

GUARD_ELEMS = 1024
_SENTINEL_BITS = {torch.float32: 0x7FE5A5A5, torch.bfloat16: 0x5A5A}  # (fp32: a quiet NaN payload; bf16: ~1.5e16)
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


class Guarded:
    """``t``: a tensor of ``shape``/``dtype`` inside a larger allocation on ``device``.  ``window`` = (off, C): only
    channels [off, off + C) of the last axis belong to the kernel's output; the rest of each row and ``guard``
    elements before and after the tensor hold the sentinel.  ``fill``: initial value of the window (scalar, or a
    tensor of the window's shape), else the sentinel; ``outside``: a value for the channels outside the window instead
    of the sentinel (they are compared bit for bit all the same)."""

    def __init__(self, shape, dtype, device, window=None, fill=None, guard=GUARD_ELEMS, outside=None):
        shape = tuple(shape)
        n = math.prod(shape)
        self.dtype, self.guard, self.shape = dtype, guard, shape
        self.base = torch.empty(guard + n + guard, dtype=dtype, device=device)
        self.base.view(_INT_VIEW[dtype]).fill_(_SENTINEL_BITS[dtype])
        self.t = self.base[guard:guard + n].view(shape)
        ctot = shape[-1]
        self.win = (0, ctot) if window is None else tuple(window)
        assert 0 <= self.win[0] and self.win[0] + self.win[1] <= ctot
        if outside is not None:
            self.t[...] = outside
        if fill is not None:
            self.window_view()[...] = fill
        keep = torch.ones(n + 2 * guard, dtype=torch.bool)
        keep[guard:guard + n].view(-1, ctot)[:, self.win[0]:self.win[0] + self.win[1]] = False
        self.mask = keep.to(device)
        self.snap = self.base.view(_INT_VIEW[dtype])[self.mask].clone()

    def window_view(self):
        return self.t[..., self.win[0]:self.win[0] + self.win[1]]

    def violations(self):
        """positions (relative to the tensor's first element) of guard elements that changed"""
        now = self.base.view(_INT_VIEW[self.dtype])[self.mask]
        diff = (now != self.snap).nonzero().flatten()
        return (self.mask.nonzero().flatten()[diff] - self.guard).cpu()


def assert_guards_intact(*bufs, label=""):
    """every guard element of every ``Guarded`` in ``bufs`` holds its sentinel, bit for bit"""
    for i, g in enumerate(bufs):
        pos = g.violations()
        if pos.numel():
            n = math.prod(g.shape)
            where = []
            for p in pos[:5].tolist():
                if p < 0:
                    where.append(f"{-p} elements before the tensor")
                elif p >= n:
                    where.append(f"{p - n} elements past its end")
                else:
                    c = []
                    for s in reversed(g.shape):
                        c.append(p % s)
                        p //= s
                    where.append(f"index {tuple(reversed(c))} outside the channel window {g.win}")
            raise AssertionError(f"{label} buffer {i}: {pos.numel()} guard elements written: " + "; ".join(where))
