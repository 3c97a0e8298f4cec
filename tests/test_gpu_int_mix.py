"""Whole-factor AREA shrinks (resizeAreaFast_) and NN frames of different geometry share launches.

k_area_int_mix / k_resize_nn_mix carry the bodies of the lone kernels behind a descriptor table, so every output here
must equal, byte for byte, what one impgpu_batch_cv_resize launch (or one impgpu_run_ops call) per frame leaves, and what
the oracle computes -- and the number of kernels enqueued must follow the kinds of frames in the call, not their number."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, _release, check_against_loop, check_against_oracle, run_both

pytestmark = pytest.mark.gpu

# (height, width) of the usual sources and the thumbnail each one shrinks to by a whole factor: 2, 3, 4, 5, 6, 7, 8, 12
STANDARD = [((480, 640), "320,240"), ((540, 960), "320,180"), ((720, 1280), "320,180"), ((900, 1600), "320,180"),
            ((1080, 1920), "320,180"), ((1260, 2240), "320,180"), ((1440, 2560), "320,180"), ((2160, 3840), "320,180")]
CANARY = 0xA5


def _standard_sources(channels):
    out = []
    for k, ((h, w), resize) in enumerate(STANDARD):
        for c in channels:
            out.append((noise_image(h, w, 3, 1100 + k) if c == 3 else smooth_image(h, w, 4, 20 + k), resize))
    return out


@pytest.mark.parametrize("channels", [(3,), (4,), (3, 4)])
def test_standard_sizes_share_one_launch(gpu, channels):
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(32, 80, 4, 1150), ("r", "b", 8, 8, 70))
    src = _standard_sources(channels)
    reqs = [Req(a, "plain", resize=resize) for a, resize in src]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("bare: %d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    for im, (_, resize) in zip(ims, src):
        w, h = (int(v) for v in resize.split(","))
        assert im.shape[:2] == (h, w), im.shape                       # (every factor is whole)
    assert launches == len(channels), launches                        # one per channel count; the loop: one per request
    _release(ims, clones)
    # with a BGRA overlay: the resize launch, then the pointwise tail all the requests share
    reqs = [Req(a, "wm", resize=resize) for a, resize in src]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("watermarked: %d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 2 * len(channels), launches
    _release(ims, clones)
    cf.release()


class Frame:
    """A source window inside a larger resident frame and a destination window inside a canary-filled one."""

    def __init__(self, torch, rng, cn, sw, sh, dw, dh, interp):
        self.cn, self.sw, self.sh, self.dw, self.dh, self.interp = cn, sw, sh, dw, dh, interp
        ox, oy, px, py = (int(v) for v in rng.integers(0, 6, size=4))      # (an odd ox: a BGRA start off the 16-byte grid)
        dpad = int(rng.integers(0, 4))
        if cn == 3 and rng.integers(0, 2) == 0:                        # BGR the streaming bodies take: 4-byte aligned rows and starts
            ox = 4 * (ox % 2)
            px += (-(sw + ox + px)) % 4
            dpad = (-dw) % 4
        self.host = rng.integers(0, 256, size=(sh + oy + py, sw + ox + px, cn), dtype=np.uint8)
        self.window = self.host[oy:oy + sh, ox:ox + sw]
        self.src = torch.from_numpy(self.host).cuda()
        self.sstep = self.host.shape[1] * cn
        self.sptr = self.src.data_ptr() + oy * self.sstep + ox * cn
        self.dsts = [torch.full((dh, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.dstep = (dw + dpad) * cn

    def item(self, which):
        return (self.sptr, self.sw, self.sh, self.sstep, self.dsts[which].data_ptr(), self.dw, self.dh, self.dstep)

    def out(self, which):
        return self.dsts[which].cpu().numpy()

    def want(self):
        return orc.cv_resize(np.ascontiguousarray(self.window), self.dw, self.dh, self.interp)


def _check_frames(gpu, frames, cn, where):
    """Destination 0 holds the batch's bytes: compare with one impgpu_batch_cv_resize launch per frame and the oracle."""
    for f in frames:
        sp, sw, sh, ss, dp, dw, dh, ds = f.item(1)
        gpu.batch_cv_resize(sp, 0, sw, sh, ss, dp, 0, dw, dh, ds, cn, 1, f.interp)
    gpu.sync()
    for i, f in enumerate(frames):
        got, each = f.out(0), f.out(1)
        assert np.array_equal(got, each), (where, i, cn, f.sw, f.sh, f.dw, f.dh)
        assert np.array_equal(got[:, :f.dw], f.want()), (where, i, cn, f.sw, f.sh, f.dw, f.dh)
        assert (got[:, f.dw:] == CANARY).all(), (where, i)


def _whole_frame(torch, rng, cn):
    isx, isy = (int(v) for v in rng.integers(1, 21, size=2))          # independent: anisotropic, 1 x k, k x 1, areas over 257
    if rng.integers(0, 8) == 0:
        isx = isy = 2                                                  # (1 in 400 otherwise)
    dw = int(rng.choice([1, 2, 3, 5, 7, 16, 33, 64, 90, int(rng.integers(1, 120))]))
    dh = int(rng.integers(1, 40))
    return Frame(torch, rng, cn, isx * dw, isy * dh, dw, dh, orc.INTER_AREA)


def _general_frame(torch, rng, cn):
    dw, dh = int(rng.integers(16, 80)), int(rng.integers(8, 40))
    while True:
        sw, sh = int(dw * rng.uniform(1.2, 5.0)), int(dh * rng.uniform(1.2, 5.0))
        if sw % dw or sh % dh:
            return Frame(torch, rng, cn, sw, sh, dw, dh, orc.INTER_AREA)


@pytest.mark.parametrize("seed", range(6))
def test_direct_api_fuzz(gpu, seed):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D7100 + seed))
    for cn in (1, 3, 4):
        n = int(rng.integers(2, 49))
        frames, general = [], 0
        for k in range(n):
            if k >= 2 and rng.integers(0, 5) == 0:                     # non-whole shrinks ride in the same call
                frames.append(_general_frame(torch, rng, cn))
                general += 1
            else:
                frames.append(_whole_frame(torch, rng, cn))
        torch.cuda.synchronize()
        rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
        assert rc == 0
        # kernel groups present: the whole-factor frames, the general shrinks (gray ones are not gathered: one each)
        groups = 1 + ((1 if general else 0) if cn != 1 else general)
        print("seed %d cn %d: %d frames (%d general), %d launches, %d groups" % (seed, cn, n, general, launches, groups))
        assert 1 <= launches <= groups, (cn, n, general, launches)
        _check_frames(gpu, frames, cn, "fuzz seed %d" % seed)


def test_a_lone_whole_factor_frame_keeps_its_lone_launch(gpu):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D7200))
    for cn in (1, 3, 4):
        one = [Frame(torch, rng, cn, 4 * 60, 4 * 30, 60, 30, orc.INTER_AREA)]
        torch.cuda.synchronize()
        rc, launches = gpu.batch_resize_mixed([f.item(0) for f in one], cn, count_launches=True)
        assert (rc, launches) == (0, 1)
        _check_frames(gpu, one, cn, "lone")
    # ... also among general shrinks, which share the other launch
    frames = [_general_frame(torch, rng, 4) for _ in range(3)] + [Frame(torch, rng, 4, 3 * 50, 5 * 20, 50, 20, orc.INTER_AREA)]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], 4, count_launches=True)
    assert (rc, launches) == (0, 2)
    _check_frames(gpu, frames, 4, "lone among general")


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_nn_frames_share_one_launch(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D7300 + cn))
    for n in (2, 9, 32):
        frames = []
        for _ in range(n):
            sw, sh, dw, dh = (int(v) for v in rng.integers(1, 200, size=4))    # shrinks and enlargements alike
            frames.append(Frame(torch, rng, cn, sw, sh, dw, dh, orc.INTER_NN))
        torch.cuda.synchronize()
        rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, simple=True, count_launches=True)
        assert (rc, launches) == (0, 1), (n, rc, launches)
        _check_frames(gpu, frames, cn, "nn %d" % n)


def test_simple_requests_share_one_launch_per_channel_count(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    reqs = []
    for k in range(12):
        h, w = 300 + 37 * k, 420 + 53 * k
        a = noise_image(h, w, 3, 1200 + k) if k % 2 else smooth_image(h, w, 4, 40 + k)
        reqs.append(Req(a, "plain", resize="%d,0" % (120 + 11 * k), simple=1))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 2, launches
    _release(ims, clones)
    cf.release()


@pytest.mark.parametrize("bad", ["null_dst", "zero_width", "unaligned_bgra_step"])
def test_a_malformed_item_launches_nothing(gpu, bad):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D7400))
    frames = [Frame(torch, rng, 4, 3 * 40, 3 * 20, 40, 20, orc.INTER_AREA) for _ in range(5)]
    frames += [_general_frame(torch, rng, 4) for _ in range(2)]
    torch.cuda.synchronize()
    items = [list(f.item(0)) for f in frames]
    if bad == "null_dst":
        items[3][4] = 0
    elif bad == "zero_width":
        items[3][1] = 0
    else:
        items[3][3] += 2                                               # BGRA rows must be 4-byte aligned
    rc, launches = gpu.batch_resize_mixed([tuple(it) for it in items], 4, count_launches=True)
    gpu.sync()
    assert rc == gpu.IMP_ERROR_INVALID_ARGS and launches == 0, (rc, launches)
    for f in frames:
        assert (f.out(0) == CANARY).all()


def test_large_batch(gpu):
    """256 whole-factor requests, BGR and BGRA, a third of them watermarked.  The oracle checks a sample: every request
    whose index is a multiple of 7 (37 of them; 7 is coprime to the 8 sizes and the 2 channel counts, so every size and
    both channel counts are in it)."""
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(40, 96, 4, 1300), ("r", "b", 10, 10, 55))
    src = _standard_sources((3, 4))
    reqs = [Req(src[k % len(src)][0], "wm" if k % 3 == 0 else "plain", resize=src[k % len(src)][1]) for k in range(256)]
    res, launches, ims, _, _ = run_both(gpu, cf, reqs, compare_loop=False)
    sample = [i for i in range(len(reqs)) if i % 7 == 0]
    assert len(sample) >= 32
    assert all(r == (0, 7) for r in res), [r for r in res if r != (0, 7)][:4]
    check_against_oracle(cf, reqs, res, ims, skip=set(range(len(reqs))) - set(sample))
    print("large batch: %d requests, %d launches" % (len(reqs), launches))
    assert launches < 8, launches                                      # the loop: one or two for each of 256 requests
    _release(ims)
    cf.release()
