"""Enlargements through impgpu_batch_run_ops: the resize round hands them to launch_resize_mixed, where the BGR and the BGRA
ones of a call share one k_resize_up_cubic_mix launch each.  Every request must come out as the per-request loop of
impgpu_run_ops leaves it and as the oracle chain makes it."""
import pytest

from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, _release, check_against_loop, check_against_oracle, run_both

pytestmark = pytest.mark.gpu


def _small(k, c):
    """Source k of 12: 60..115 wide, 40..62 high -- enlarged to 130 + 10 k wide it stays under 300 x 150."""
    h, w = 40 + 2 * k, 60 + 5 * k
    return noise_image(h, w, c, 3100 + k) if c != 4 else smooth_image(h, w, 4, 90 + k)


def _enlargements(cfg):
    reqs = [Req(_small(k, 3 + k % 2), cfg, resize="%d,0,up" % (130 + 10 * k)) for k in range(12)]
    for r in reqs:
        h, w = r.src.shape[:2]
        tw = int(r.job["resize"].split(",")[0])
        assert 40 <= min(h, w) and max(h, w) <= 120 and 130 <= tw <= 260 and h * tw / w <= 150
    return reqs


def test_bare_enlargements_share_one_launch_per_channel_count(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(20, 50, 4, 3150), ("r", "b", 4, 4, 70))
    reqs = _enlargements("plain")
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("bare: %d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(im.shape[1] > r.src.shape[1] and im.shape[0] > r.src.shape[0] for im, r in zip(ims, reqs))
    assert launches == 2, launches                                     # the loop: 12
    _release(ims, clones)
    # with a BGRA overlay: the resize launch, then the tail all the requests of a channel count share
    reqs = _enlargements("wm")
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("watermarked: %d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 4, launches
    _release(ims, clones)
    cf.release()


def test_enlargements_shrinks_and_a_gray_enlargement(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    reqs, classes = [], set()
    for k in range(12):
        c = 3 + k % 2
        if k % 3 == 2:                                                 # a general shrink: 181 + 23 k wide to 50 + k, never a whole factor
            h, w, tw = 90 + 7 * k, 181 + 23 * k, 50 + k
            assert w % tw and tw < w
            a = noise_image(h, w, 3, 3200 + k) if c == 3 else smooth_image(h, w, 4, 95 + k)
            reqs.append(Req(a, "plain", resize="%d,0" % tw))
            classes.add((c, "rows"))
        else:
            reqs.append(Req(_small(k, c), "plain", resize="%d,0,up" % (130 + 10 * k)))
            classes.add((c, "up"))
    reqs.insert(5, Req(_small(5, 1), "plain", resize="170,0,up"))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("mix: %d requests, %d launches, classes %s" % (len(reqs), launches, sorted(classes)))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    # one launch per class present per channel count; the gray enlargement: its own resize launch and its promotion
    assert len(classes) == 4
    assert launches == len(classes) + 2, launches
    _release(ims, clones)
    cf.release()


def test_resize_fault_point_among_enlargements(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    reqs = _enlargements("plain")[:8]
    step, target = 4, 2                                                # IMP_STEP_RESIZE; every request enters it, in order
    lib = gpu.lib
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims]
    try:
        assert lib.impgpu_fault_arm(step, target + 1) == 0
        res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        assert lib.impgpu_fault_arm(step, target + 1) == 0
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    finally:
        lib.impgpu_fault_arm(-1, 0)
    failed = [i for i, r in enumerate(res) if r[0] != 0]
    assert failed == [target], res
    assert res[target] == (gpu.IMP_ERROR_DEVICE, step) and loop[target] == res[target]
    assert ims[target].shape == reqs[target].src.shape                 # it keeps its frame
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims, skip=failed)
    _release(ims, clones)
    cf.release()
