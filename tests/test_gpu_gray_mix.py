"""Gray frames on the batched path: general INTER_AREA shrinks of gray frames share one k_resize_area_mix<1> launch, and
gray requests ride impgpu_batch_run_ops' shared launches (resize -> one promotion launch -> the 3-channel groups).

Every output must equal, byte for byte, what one launch (or one impgpu_run_ops call) per frame leaves and what the oracle
computes; the number of kernels enqueued must follow the kinds of frames in the call, not their number."""
import math

import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, _release, check_against_loop, check_against_oracle, run_both
from test_gpu_int_mix import CANARY, Frame, _check_frames

pytestmark = pytest.mark.gpu

WINDOW_LIMIT = 20            # source columns the mixed body's window holds (include/impgpu.h)

# (sw, sh, dw, dh): each the smallest that reaches its corner of the body
NAMED = [(37, 29, 17, 13),        # one partial strip
         (100, 75, 64, 63),       # factor 1.56: windows of 2-3, exactly one full strip
         (200, 31, 65, 9),        # a 64-column strip plus a one-column strip
         (513, 300, 100, 77),     # width not a multiple of 4: pitch padding
         (1279, 7, 640, 3),       # factor 1.998: many strips, fewer rows than a band
         (640, 480, 224, 168),    # the workload's small cousin
         (10, 7, 3, 2),           # a row shorter than one 16-byte granule
         (5, 300, 3, 17),         # tall narrow cells
         (128, 45, 64, 20),       # whole factor on x only
         (1000, 40, 53, 7)]       # 18.9x: the widest window


def widest_cell(ssize, dsize):
    """Source pixels the widest destination cell touches (computeResizeAreaTab's arithmetic, in Python's doubles)."""
    scale = 1.0 / (dsize / ssize)
    most = 0
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        s1, s2 = math.ceil(f1), min(math.floor(f2), ssize - 1)
        s1 = min(s1, s2)
        most = max(most, (s2 - s1) + (1 if s1 - f1 > 1e-3 else 0) + (1 if f2 - s2 > 1e-3 else 0))
    return most


class GrayFrame(Frame):
    """test_gpu_int_mix.Frame for one channel with a chosen source alignment: the window starts `shift` bytes past a
    4-byte boundary inside a frame whose pitch is whatever the padding makes it; the destination rows are 4-byte aligned
    unless `dst_unaligned`."""

    def __init__(self, torch, rng, sw, sh, dw, dh, shift=None, dst_unaligned=False, interp=None):
        self.cn, self.sw, self.sh, self.dw, self.dh = 1, sw, sh, dw, dh
        self.interp = orc.INTER_AREA if interp is None else interp
        oy, px, py = (int(v) for v in rng.integers(0, 6, size=3))
        ox = int(rng.integers(0, 6))
        if shift is not None:                                          # (torch's allocations start on a 256-byte boundary)
            ox, px = next((o, q) for o in range(4) for q in range(4) if (oy * (sw + o + q) + o) % 4 == shift)
        dpad = (-dw) % 4
        if dst_unaligned:
            dpad += 1 + int(rng.integers(0, 3))                        # (dw + dpad) % 4 is 1, 2 or 3
        self.host = rng.integers(0, 256, size=(sh + oy + py, sw + ox + px, 1), dtype=np.uint8)
        self.window = self.host[oy:oy + sh, ox:ox + sw]
        self.src = torch.from_numpy(self.host).cuda()
        self.sstep = self.host.shape[1]
        self.sptr = self.src.data_ptr() + oy * self.sstep + ox
        if shift is not None:
            assert self.sptr % 4 == shift
        self.dsts = [torch.full((dh, dw + dpad, 1), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.dstep = dw + dpad
        self.lone_by_rule = bool(self.dstep % 4) or sw / dw > 16 or sh / dh > 16


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_named_shapes_share_one_launch(gpu, shift):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D8100 + shift))
    frames = [GrayFrame(torch, rng, sw, sh, dw, dh, shift=shift) for sw, sh, dw, dh in NAMED]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], 1, count_launches=True)
    assert rc == 0
    wide = widest_cell(1000, 53)
    print("shift %d: %d frames, %d launches (widest cell of 1000 -> 53: %d columns)" % (shift, len(frames), launches, wide))
    assert launches <= 2, launches                 # the mixed launch, plus at most the 18.9x frame alone
    if wide <= WINDOW_LIMIT:
        assert launches == 1, launches
    _check_frames(gpu, frames, 1, "named, shift %d" % shift)


@pytest.mark.parametrize("seed", range(6))
def test_gray_fuzz(gpu, seed):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D8200 + seed))
    n = int(rng.integers(2, 49))
    frames = []
    for k in range(n):
        if k % 6 == 3:                                                 # whole-factor frames ride in the same call
            isx, isy = (int(v) for v in rng.integers(1, 13, size=2))
            dw, dh = int(rng.integers(1, 90)), int(rng.integers(1, 20))
            frames.append(GrayFrame(torch, rng, isx * dw, isy * dh, dw, dh))
            continue
        dw = int(rng.choice([1, 2, 3, 5, 63, 64, 65, int(rng.integers(1, 200))]))
        dh = int(rng.integers(2, 14))                                  # (two rows: some height is no multiple of it)
        while True:
            sw, sh = int(dw * rng.uniform(1.05, 16)), int(dh * rng.uniform(1.05, 16))
            if sw >= dw and sh >= dh and (sw % dw or sh % dh):
                break
        frames.append(GrayFrame(torch, rng, sw, sh, dw, dh, dst_unaligned=(k % 5 == 4)))
    torch.cuda.synchronize()
    lone = sum(f.lone_by_rule for f in frames)                         # from geometry alone: factor > 16, unaligned destination
    assert 4 * lone <= n, (lone, n)
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], 1, count_launches=True)
    assert rc == 0
    print("seed %d: %d frames, %d lone by the rule, %d launches" % (seed, n, lone, launches))
    assert 1 <= launches <= 2 + lone, (n, lone, launches)              # general shrinks, whole factors, the lone ones
    # what the body promises beyond the rule: it stores to any destination alignment, so with every factor at most 16
    # nothing goes alone
    assert all(f.sw / f.dw <= 16 and f.sh / f.dh <= 16 for f in frames)
    assert launches <= 2, (n, launches)
    _check_frames(gpu, frames, 1, "gray fuzz seed %d" % seed)


def test_launch_counts(gpu):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D8300))
    two = [GrayFrame(torch, rng, 301, 203, 120, 81), GrayFrame(torch, rng, 777, 500, 224, 144)]
    one = [GrayFrame(torch, rng, 640, 480, 224, 168)]
    nn = [GrayFrame(torch, rng, *(int(v) for v in rng.integers(1, 200, size=4)), interp=orc.INTER_NN) for _ in range(32)]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in two], 1, count_launches=True)
    assert (rc, launches) == (0, 1), (rc, launches)                    # (one each before gray frames were gathered)
    _check_frames(gpu, two, 1, "two")
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in one], 1, count_launches=True)
    assert (rc, launches) == (0, 1), (rc, launches)                    # alone: the lone kernel
    _check_frames(gpu, one, 1, "one")
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in nn], 1, simple=True, count_launches=True)
    assert (rc, launches) == (0, 1), (rc, launches)
    _check_frames(gpu, nn, 1, "nn")


# ---------------------------------------------------------------- gray requests through impgpu_batch_run_ops
def _gray_thumbs(n):
    """n gray sources of n different sizes (test_gpu_batch_ops._thumbs' sizes), none an integer multiple of a thumbnail's."""
    return [smooth_image(401 + 61 * k, 617 + 97 * k, 1, k) if k % 2 else noise_image(401 + 61 * k, 617 + 97 * k, 1, 2000 + k)
            for k in range(n)]


def _configs(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(30, 76, 4, 2050), ("r", "b", 6, 4, 70))                 # a BGRA overlay
    cf.add("wm3", noise_image(26, 50, 3, 2051), ("l", "t", 3, 2, 45))                # a BGR overlay
    return cf


# (config, job, launches of a call made of such requests alone).  Every call: ONE resize launch (k_resize_area_mix<1>)
# and ONE promotion launch (k_gray2bgr_mix); then the chain's segments, each one launch for all its requests -- a gray
# frame's turn never rides its resize, and its overlay is always the tail's.
GRAY_CHAINS = [
    ("plain", dict(resize="224,0"), 2),                                              # no segment
    ("plain", dict(crop="1,1,c,c", resize="120,0"), 2),                              # a window at an odd byte
    ("plain", dict(resize="224,0", filters=["gamma=1.4"]), 3),                       # + the pointwise tail
    ("plain", dict(resize="224,0", filters=["rotate=90"]), 3),                       # + k_geom_mix<3>
    ("plain", dict(resize="224,0", filters=["blur=1.5"]), 3),                        # + k_blur_mix<3, ...> (one form)
    ("wm", dict(resize="224,0"), 3),                                                 # + the tail: the overlay alone
    ("wm3", dict(resize="224,0"), 3),
    ("wm", dict(resize="224,0", filters=["modulate=100,0,100"]), 3),                 # + the tail: run and overlay in one
]


@pytest.mark.parametrize("kind", range(len(GRAY_CHAINS)))
def test_gray_requests_share_launches(gpu, kind):
    cf = _configs(gpu)
    cfg, job, expect = GRAY_CHAINS[kind]
    reqs = [Req(a, cfg, **job) for a in _gray_thumbs(16)]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("%s %s: %d requests, %d launches" % (cfg, job, len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(im.shape[2] == 3 for im in ims)
    segments = expect - 2
    assert launches <= 3 + 1 + segments * 1                            # the issue's bound: resizes, promotion, segments x kinds
    assert launches == expect, (launches, expect)                      # the loop: two to four launches for each of 16
    _release(ims, clones)
    cf.release()


def test_gray_filtered_mix_shares_launches(gpu):
    cf = _configs(gpu)
    src = _gray_thumbs(16)
    reqs = [Req(a, GRAY_CHAINS[k % len(GRAY_CHAINS)][0], **GRAY_CHAINS[k % len(GRAY_CHAINS)][1]) for k, a in enumerate(src)]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("filtered mix: %d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    # one resize launch (all general shrinks), the promotion, and round 1 of every chain: the pointwise / tail launch, the
    # turn's and the blur's.  No chain here has a second segment: 1 + 1 + 1 x 3.
    assert launches <= 3 + 1 + 1 * 3
    assert launches == 5, launches
    _release(ims, clones)
    cf.release()


def test_gray_requests_join_the_bgr_groups(gpu):
    """Gray, BGR and BGRA requests with the same filter lists: the gray ones cost their resize and their promotion, and not
    one segment launch more."""
    cf = _configs(gpu)
    chains = [("plain", ["gamma=1.4"]), ("plain", ["blur=1.5"]), ("plain", ["flip=10", "gamma=1.2"]), ("wm", ["modulate=100,0,100"])]
    colour, gray = [], []
    for k in range(8):
        cfg, filters = chains[k % len(chains)]
        h, w = 431 + 53 * k, 643 + 89 * k
        colour.append(Req(noise_image(h, w, 3, 2100 + k), cfg, resize="224,0", filters=filters))
        colour.append(Req(smooth_image(h + 7, w + 11, 4, 70 + k), cfg, resize="224,0", filters=filters))
        gray.append(Req(noise_image(h + 3, w + 5, 1, 2150 + k), cfg, resize="224,0", filters=filters))
    res, without, ims, clones, loop = run_both(gpu, cf, colour)
    check_against_loop(res, ims, clones, loop)
    _release(ims, clones)
    reqs = [r for trio in zip(colour[0::2], gray, colour[1::2]) for r in trio]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("colour alone: %d launches; with %d gray requests: %d" % (without, len(gray), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == without + 2, (without, launches)
    _release(ims, clones)
    cf.release()


# request: (channels, job); every request uses the watermarked config
FAULT_REQS = [(1, dict(resize="224,0")),
              (3, dict(resize="224,0")),
              (1, dict(resize="200,0", filters=["gamma=1.3"])),
              (4, dict(resize="200,0", filters=["gamma=1.3"])),
              (1, dict(crop="1,1,c,c", resize="180,0")),
              (3, dict(resize="210,0", filters=["blur=1.5"])),
              (1, dict(resize="0,150", filters=["rotate=90"])),
              (1, dict(resize="190,0", simple=1))]


@pytest.mark.parametrize("step,target", [(4, 0), (4, 2), (4, 5), (5, 0), (5, 2), (5, 3), (5, 4), (5, 7), (6, 0), (6, 6), (3, 4)])
def test_fault_points_cut_the_same_gray_request(gpu, step, target):
    cf = _configs(gpu)
    reqs = []
    for k, (c, job) in enumerate(FAULT_REQS):
        h, w = 401 + 41 * k, 617 + 59 * k
        a = smooth_image(h, w, 4, 80 + k) if c == 4 else noise_image(h, w, c, 2200 + k)
        reqs.append(Req(a, "wm", **job))
    # the requests that enter the step, in order: CROP with a crop; RESIZE and WATERMARK all of them; FILTERING with filters
    # -- and every gray request, for its promotion (bridge.c:613-618)
    entering = [i for i, (c, job) in enumerate(FAULT_REQS)
                if (step != 3 or "crop" in job) and (step != 5 or c == 1 or job.get("filters"))]
    nth = entering.index(target) + 1
    lib = gpu.lib
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims]
    try:
        assert lib.impgpu_fault_arm(step, nth) == 0
        res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        assert lib.impgpu_fault_arm(step, nth) == 0
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    finally:
        lib.impgpu_fault_arm(-1, 0)
    failed = [i for i, r in enumerate(res) if r[0] != 0]
    assert failed == [target], res
    assert res[target] == (gpu.IMP_ERROR_DEVICE, step)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims, skip=failed)
    if FAULT_REQS[target][0] == 1:
        # a gray request cut at FILTERING keeps its resized GRAY frame; cut at WATERMARK, the promoted and filtered one
        want_c = {3: 1, 4: 1, 5: 1, 6: 3}[step]
        assert ims[target].shape[2] == want_c, (ims[target].shape, step)
        if step == 5:
            job = FAULT_REQS[target][1]
            rc, _, want = cf.oracle(Req(reqs[target].src, "plain", **{k: v for k, v in job.items() if k != "filters"}), reqs[target].src)
            assert rc == 0 and want.shape[2] == 3
            got = ims[target].numpy()
            assert got.shape[:2] == want.shape[:2] and np.array_equal(got[:, :, 0], want[:, :, 0])
    _release(ims, clones)
    cf.release()
