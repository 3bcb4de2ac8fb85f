"""[CONSISTENCY_LOSS] under data parallelism (CPU, gloo, two ranks): the term is a plain mean over samples, so with
the section on the two-rank generator iteration equals the single-process iteration on the full batch - loss value and
post-step generator weights - with no collective of its own.  Helpers and tolerance of tests/test_dist_gloo.py.

Both sides run in float64, for the reason tests/test_distribution_loss_dist.py gives: what is compared is Adam's FIRST
step, w - lr g / (|g| + eps), which magnifies the difference of the two summation orders (the ranks' all-reduce against
the batch sum of one backward pass) for the handful of elements whose gradient is near eps = 1e-8; in float64 that
difference is 1e-18 and the tolerance tests the algebra: that the term is a plain mean over samples."""
import os

import numpy as np
import torch
import torch.multiprocessing as mp

from conftest import REPO
from test_dist_gloo import _build_gan, _free_port, _g_iteration

SECTION = dict(present=True, weight=0.5, kernel="box", sigma=None, factor=0, norm="l1")


def _gan_with_section(on=True):
    torch.set_default_dtype(torch.float64)
    try:
        gan, cfg = _build_gan()
    finally:
        torch.set_default_dtype(torch.float32)
    gan.G.double()
    gan.D.double()
    for k, v in SECTION.items():  # (after the build: Config() resets the class-level section)
        setattr(cfg.consistency_loss, k, v if on else getattr(type(cfg.consistency_loss), k))
    return gan, cfg


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from gan_sr_wind_field_amd import dist as wdist
    from oracle.gan import synthetic_batch

    assert wdist.init_from_env("gloo")
    out = {}
    for tag, on in (("plain", False), ("consistency", True)):
        gan, cfg = _gan_with_section(on)
        dp = wdist.attach(gan, bucket_mb=0.05, sync_bn=True)
        LR, HR, Z, x, y = (t.double() for t in synthetic_batch(world, 16, 4, 4, seed=2001))
        sl = slice(rank, rank + 1)  # one sample per rank
        w, losses = _g_iteration(gan, cfg, LR[sl], HR[sl], Z[sl], x, y)
        out[tag] = {"w": w, "losses": losses, "n_coll": dp.n_collectives}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_g_iteration_with_the_section_equals_full_batch(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from oracle.gan import synthetic_batch

    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "rank0.pt")
    r1 = torch.load(tmp_path / "rank1.pt")
    try:
        gan, cfg = _gan_with_section()
        LR, HR, Z, x, y = (t.double() for t in synthetic_batch(world, 16, 4, 4, seed=2001))
        w_ref, losses_ref = _g_iteration(gan, cfg, LR, HR, Z, x, y)
        gan_p, cfg_p = _gan_with_section(False)
        w_plain, _ = _g_iteration(gan_p, cfg_p, LR, HR, Z, x, y)
    finally:
        _gan_with_section(False)
    assert losses_ref["consistency"] > 0 and "consistency" not in r0["plain"]["losses"]
    for k, v in w_ref.items():
        # both ranks end with the same weights, equal to the single-process step on the full batch
        assert torch.equal(r0["consistency"]["w"][k], r1["consistency"]["w"][k]), k
        np.testing.assert_allclose(r0["consistency"]["w"][k].numpy(), v.numpy(), rtol=2e-5, atol=1e-7, err_msg=k)
    assert any(not torch.equal(w_ref[k], w_plain[k]) for k in w_ref)  # the term moved the step
    # a plain mean over samples: the average over ranks of the per-rank means is the full-batch mean, as for pix
    np.testing.assert_allclose(0.5 * (r0["consistency"]["losses"]["consistency"] + r1["consistency"]["losses"]["consistency"]),
                               losses_ref["consistency"], rtol=1e-5)
    np.testing.assert_allclose(0.5 * (r0["consistency"]["losses"]["pix"] + r1["consistency"]["losses"]["pix"]), losses_ref["pix"], rtol=1e-5)
    for r in (r0, r1):  # no collective of its own
        assert r["consistency"]["n_coll"] == r["plain"]["n_coll"]
