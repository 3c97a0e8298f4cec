"""INTER_AREA shrinks whose cells span 21..66 source columns (factors past 18x, up to 64x) of BGR / BGRA frames:
k_resize_area_wide alone and in uniform batches, k_resize_area_wide_mix for frames of different geometry in one launch.

Every output must equal, byte for byte, what one impgpu_batch_cv_resize launch per frame leaves and what the oracle computes
(itself pinned on these shapes by test_oracle_wide_area); the number of kernels enqueued must follow the kinds of frames in
the call, not their number.  BGR sources here have 4-byte aligned rows and starts (what cvCreateImage makes): the rule of
the wide kernels asks for them, and an unaligned one keeps k_resize_area and its tables."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from test_gpu_batch_ops import Configs, Req, _release, check_against_loop, check_against_oracle, run_both
from test_gpu_gray_mix import widest_cell
from test_gpu_int_mix import CANARY, Frame, _check_frames, _general_frame
from test_oracle_wide_area import SHAPES

pytestmark = pytest.mark.gpu

W_MIN, W_MAX = 21, 66        # widest horizontal cell the wide kernels take (include/impgpu.h)

# SHAPES, and what each one hits
#   (1401, 40) -> (70, 3)      W = 21, the first width past the bodies with compile-time windows; two strips, the second partial
#   (1331, 40) -> (70, 3)      W = 20: still the old path
#   (605, 90) -> (30, 7)       20.17x by 12.9x, one partial strip
#   (1009, 45) -> (37, 5)      27.3x, whole y factor (9)
#   (1300, 60) -> (33, 3)      39.4x by exactly 20
#   (2509, 50) -> (130, 17)    three strips, two bands (dh > 16)
#   (1261, 37) -> (64, 37)     y untouched (factor 1), one full strip
#   (700, 900) -> (30, 20)     tall cells (45 rows)
#   (50, 7) -> (1, 2)          one column, W = sw = 50
#   (4090, 9) -> (64, 2)       W = 65, the longest line
#   (4200, 9) -> (64, 2)       W = 67, past the rule: the table kernel
#   (1210, 403) -> (60, 20)    a phone photo's factors at a tenth of the pixels
OLD_PATH, PAST_RULE = (1331, 40, 70, 3), (4200, 9, 64, 2)
ACCEPTED = [s for s in SHAPES if s not in (OLD_PATH, PAST_RULE)]
# BGR only: sw * 3 is no multiple of 4 and the last strip's window ends at the row's end -- the ragged last granule, with the
# frame ending where the row's padding ends
RAGGED = (1403, 11, 70, 2)


def test_the_shapes_are_what_they_claim():
    assert len(ACCEPTED) == 10
    assert widest_cell(1401, 70) == 21 and widest_cell(1331, 70) == 20
    assert widest_cell(50, 1) == 50 and widest_cell(4090, 64) == 65 and widest_cell(4200, 64) == 67
    assert all(W_MIN <= widest_cell(sw, dw) <= W_MAX for sw, _, dw, _ in ACCEPTED + [RAGGED])
    assert (RAGGED[0] * 3) % 4


class WideFrame(Frame):
    """test_gpu_int_mix.Frame whose BGR rows and starts are always 4-byte aligned.  `tight`: the window starts the frame and
    ends it, but for the pixels that pad a row to 4 bytes."""

    def __init__(self, torch, rng, cn, sw, sh, dw, dh, tight=False):
        self.cn, self.sw, self.sh, self.dw, self.dh, self.interp = cn, sw, sh, dw, dh, orc.INTER_AREA
        ox, oy, px, py = (int(v) for v in rng.integers(0, 6, size=4))      # (an odd ox: a BGRA start off the 16-byte grid)
        dpad = int(rng.integers(0, 4))
        if cn == 3:
            ox = 4 * (ox % 2)
            px += (-(sw + ox + px)) % 4
        if tight:
            ox, oy, py, px = 0, 0, 0, ((-sw) % 4 if cn == 3 else 0)
        self.host = rng.integers(0, 256, size=(sh + oy + py, sw + ox + px, cn), dtype=np.uint8)
        self.window = self.host[oy:oy + sh, ox:ox + sw]
        self.src = torch.from_numpy(self.host).cuda()
        self.sstep = self.host.shape[1] * cn
        self.sptr = self.src.data_ptr() + oy * self.sstep + ox * cn
        assert self.sptr % 4 == 0 and self.sstep % 4 == 0
        self.dsts = [torch.full((dh, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.dstep = (dw + dpad) * cn


def _shapes(cn):
    return SHAPES + ([RAGGED] if cn == 3 else [])


# ---------------------------------------------------------------- 1. alone and in uniform batches
@pytest.mark.parametrize("cn", [3, 4])
def test_lone_launch(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D9100 + cn))
    frames = [WideFrame(torch, rng, cn, *s, tight=(s == RAGGED)) for s in _shapes(cn)]
    torch.cuda.synchronize()
    for f in frames:
        sp, sw, sh, ss, dp, dw, dh, ds = f.item(0)
        gpu.batch_cv_resize(sp, 0, sw, sh, ss, dp, 0, dw, dh, ds, cn, 1, orc.INTER_AREA)
    _check_frames(gpu, frames, cn, "lone")                             # (the oracle, the canaries; a second launch leaves the same)


@pytest.mark.parametrize("cn", [3, 4])
def test_uniform_batch_of_nine(gpu, cn):
    import torch

    count = 9                                                          # one full group of 8 frames and a padded one
    rng = np.random.Generator(np.random.PCG64(0x1A4D9200 + cn))
    for sw, sh, dw, dh in _shapes(cn):
        pad = (-sw) % 4 if cn == 3 else int(rng.integers(0, 3))
        gap, dpad = int(rng.integers(0, 3)), int(rng.integers(0, 4))  # rows between the frames; canary columns
        host = rng.integers(0, 256, size=(count, sh + gap, sw + pad, cn), dtype=np.uint8)
        src = torch.from_numpy(host).cuda()
        dst = torch.full((count, dh, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sstep, dstep = (sw + pad) * cn, (dw + dpad) * cn
        gpu.batch_cv_resize(src.data_ptr(), (sh + gap) * sstep, sw, sh, sstep, dst.data_ptr(), dh * dstep, dw, dh, dstep, cn, count,
                            orc.INTER_AREA)
        gpu.sync()
        got = dst.cpu().numpy()
        for k in range(count):
            want = orc.cv_resize(np.ascontiguousarray(host[k, :sh, :sw]), dw, dh, orc.INTER_AREA)
            assert np.array_equal(got[k, :, :dw], want), (cn, sw, sh, dw, dh, k)
        assert (got[:, :, dw:] == CANARY).all(), (cn, sw, sh, dw, dh)


# ---------------------------------------------------------------- 2. frames of different geometry, the direct API
def _mixed(gpu, frames, cn):
    import torch

    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    assert rc == 0
    return launches


@pytest.mark.parametrize("cn", [3, 4])
def test_mixed_call_shares_one_launch(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D9300 + cn))
    wide = [WideFrame(torch, rng, cn, *s) for s in ACCEPTED]
    general = [_general_frame(torch, rng, cn) for _ in range(3)]
    whole = [Frame(torch, rng, cn, 4 * 60, 4 * 30, 60, 30, orc.INTER_AREA), Frame(torch, rng, cn, 3 * 50, 5 * 20, 50, 20, orc.INTER_AREA)]
    frames = wide[:5] + general[:2] + whole[:1] + wide[5:] + general[2:] + whole[1:]
    launches = _mixed(gpu, frames, cn)
    print("cn %d: %d frames, %d launches" % (cn, len(frames), launches))
    _check_frames(gpu, frames, cn, "mixed")
    assert launches == 3, launches                                     # wide cells, general shrinks, whole factors
    # ... and the W = 67 frame goes alone (the table kernel), the W = 20 one with the general shrinks
    for f in frames:
        f.dsts[0].fill_(CANARY)
    more = frames + [WideFrame(torch, rng, cn, *PAST_RULE), WideFrame(torch, rng, cn, *OLD_PATH)]
    launches = _mixed(gpu, more, cn)
    _check_frames(gpu, more, cn, "mixed + past the rule")
    assert launches == 4, launches
    two = [WideFrame(torch, rng, cn, *ACCEPTED[0]), WideFrame(torch, rng, cn, *ACCEPTED[-1])]
    launches = _mixed(gpu, two, cn)
    _check_frames(gpu, two, cn, "two")
    assert launches == 1, launches
    one = [WideFrame(torch, rng, cn, *ACCEPTED[3])]
    launches = _mixed(gpu, one, cn)
    _check_frames(gpu, one, cn, "one")
    assert launches == 1, launches                                     # alone: the lone launch
    old = [WideFrame(torch, rng, cn, *OLD_PATH), WideFrame(torch, rng, cn, *OLD_PATH)]
    launches = _mixed(gpu, old, cn)
    _check_frames(gpu, old, cn, "W = 20")
    assert launches == 1, launches                                     # as before: k_resize_area_mix


# ---------------------------------------------------------------- 3. a fuzz
@pytest.mark.parametrize("seed", range(6))
def test_wide_fuzz(gpu, seed):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4D9400 + seed))
    for cn in (3, 4):
        n = int(rng.integers(2, 49))
        frames = []
        for _ in range(n):
            dw, dh = int(rng.integers(1, 131)), int(rng.integers(1, 21))
            while True:
                sw, sh = int(dw * rng.uniform(19, 64)), int(dh * rng.uniform(1.05, 40))
                if sw % dw or sh % dh:                                 # (both factors whole: resizeAreaFast_, another launch)
                    break
            frames.append(WideFrame(torch, rng, cn, sw, sh, dw, dh))
        outside = sum(not W_MIN <= widest_cell(f.sw, f.dw) <= W_MAX for f in frames)
        assert 4 * outside <= n, (outside, n)
        launches = _mixed(gpu, frames, cn)
        print("seed %d cn %d: %d frames, %d outside the rule, %d launches" % (seed, cn, n, outside, launches))
        # the wide launch, the general shrinks' (cells of at most 20 columns) and one for each frame past 66
        assert 1 <= launches <= 2 + outside, (cn, n, outside, launches)
        _check_frames(gpu, frames, cn, "fuzz seed %d" % seed)


# ---------------------------------------------------------------- 4. requests through impgpu_batch_run_ops
def test_wide_requests_share_launches(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(12, 9, 4, 2300), ("r", "b", 2, 2, 70))
    reqs = []
    for k in range(16):
        w, h, dw = 1210 + (290 * k) // 15, 403 + (97 * k) // 15, 60 + (10 * k) // 15     # 1210 x 403 at 60 ... 1500 x 500 at 70
        assert W_MIN <= widest_cell(w, dw) <= W_MAX, (w, dw)
        a = noise_image(h, w, 3, 2310 + k) if k % 2 else smooth_image(h, w, 4, 90 + k)
        kind = (k // 2) % 4                                            # per channel count: four bare, two gamma, two turned
        if kind < 2:
            reqs.append(Req(a, "plain", resize="%d,0" % dw))
        elif kind == 2:
            reqs.append(Req(a, "plain", resize="%d,0" % dw, filters=["gamma=1.3"]))
        else:
            reqs.append(Req(a, "wm", resize="%d,0" % dw, filters=["rotate=90"]))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("%d requests, %d launches" % (len(reqs), launches))
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    # per channel count: ONE resize launch for its eight requests (no turn rides a wide resize: area_tail_plan's windows end
    # at 20 columns), then the chains' segments, one launch per kind and round -- round 1: the gamma run (pointwise) and the
    # turn (k_geom_mix); round 2: the turned requests' overlay (the pointwise tail)
    resize, segments = 1, 2 + 1
    assert launches == 2 * (resize + segments), launches               # (one launch per wide request before: 2 * (8 + 3))
    _release(ims, clones)
    cf.release()
