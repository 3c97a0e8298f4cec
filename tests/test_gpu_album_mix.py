"""Albums in impgpu_batch_run_ops: every frame of a BGR / BGRA album is an item of its own in the shared launches of its request's
group, the album planned once per request.

Every frame of every answer must equal, byte for byte, what impgpu_run_ops leaves on a clone of the same album and what the
oracle's chain makes of that frame; the handle stays one album with its frame count; the fault points are entered once per
request; and N albums cost the launches their frames would cost as single images, not N times the chain's length."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from test_gif import random_album
from test_gpu_batch_ops import Configs, Req, _pixels, check_against_loop, check_against_oracle, run_both

pytestmark = pytest.mark.gpu

TWO_PASS_SIGMA = 6           # blur=6 on the BGRA frames below: impgpu_blur_form 3 (checked in the test)
STEP_RESIZE, STEP_WATERMARK = 4, 6


class GifReq(Req):
    """A request whose source is a GIF: composed on the device into one BGRA album (gif_compose(album=True)); `src` holds the
    oracle's frames of the same pages."""

    def __init__(self, pages, destructive, cfg, **job):
        rc, frames = orc.gif_compose(pages, destructive)
        assert rc == 0
        Req.__init__(self, frames, cfg, **job)
        self.pages, self.destructive = pages, destructive

    def image(self, gpu):
        rc, im = gpu.gif_compose(self.pages, self.destructive, album=True)
        assert rc == 0 and im.count == len(self.src)
        return im


def _release(*groups):
    for g in groups:
        for im in g or ():
            im.release()


def _configs(gpu):
    cf = Configs(gpu)
    cf.add("plain", allow_experiments=True)
    cf.add("wm", noise_image(6, 9, 4, 5000), ("r", "b", 2, 1, 60), allow_experiments=True)      # a BGRA overlay
    return cf


# six albums of 2 to 5 frames between 20 x 9 and 64 x 48: four GIFs (BGRA), two BGR albums whose rows are padded (99 -> 100
# and 150 -> 152 bytes); and four single frames.  (kind, frames, width, height)
SOURCES = [("gif", 2, 20, 9), ("gif", 5, 37, 23), ("gif", 3, 64, 48), ("gif", 4, 50, 30), ("bgr", 3, 33, 21), ("bgr", 2, 50, 30),
           ("one4", 1, 45, 31), ("one3", 1, 33, 21), ("one4", 1, 64, 48), ("one3", 1, 41, 27)]

# what each source is asked, in two calls: between them every job kind lands on an album
NN = dict(resize="16,0", simple=1)
AREA_WM_FLAT = ("wm", dict(resize="20,0", need_flatten=1))
CROP = dict(crop="16,9")
CROP_GAMMA = dict(crop="4,3", filters=["gamma=1.4"])
AREA_TURN = dict(resize="30,0", filters=["rotate=90"])
FLIP = dict(filters=["flip=10"])
ONE_PASS = dict(filters=["blur=1.5"])
TWO_PASS = dict(filters=["blur=%d" % TWO_PASS_SIGMA])
CUBIC = dict(resize="100,0,up")
CALLS = [
    [NN, AREA_WM_FLAT, TWO_PASS, TWO_PASS, CROP, AREA_TURN, FLIP, CROP_GAMMA, ONE_PASS, CUBIC],
    [CROP_GAMMA, FLIP, ONE_PASS, CUBIC, ("wm", AREA_TURN), NN, AREA_WM_FLAT, TWO_PASS, TWO_PASS, CROP],
]


def _requests(jobs):
    reqs = []
    for k, ((kind, frames, w, h), job) in enumerate(zip(SOURCES, jobs)):
        cfg, job = job if isinstance(job, tuple) else ("plain", job)
        if kind == "gif":
            reqs.append(GifReq(random_album(5100 + k, frames, w, h), bool(k & 1), cfg, **job))
        elif kind == "bgr":
            reqs.append(Req([noise_image(h, w, 3, 5200 + 10 * k + f) for f in range(frames)], cfg, **job))
        else:
            reqs.append(Req(smooth_image(h, w, 4, 50 + k) if kind == "one4" else noise_image(h, w, 3, 5300 + k), cfg, **job))
    return reqs


@pytest.mark.parametrize("call", [0, 1])
def test_album_frames_in_shared_launches_match_loop_and_oracle(gpu, call):
    for w, h in ((64, 48), (50, 30)):
        assert gpu.blur_form(w, h, 4, TWO_PASS_SIGMA)[0] == 3 and gpu.blur_form(w, h, 4, 1.5)[0] in (1, 2)
    cf = _configs(gpu)
    reqs = _requests(CALLS[call])
    assert sum(isinstance(r.src, list) for r in reqs) == 6
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    print("call %d: %d requests, %d frames, %d launches" % (call, len(reqs), sum(im.count for im in ims), launches))
    assert all(r == (0, 7) for r in res), res
    for r, im in zip(reqs, ims):
        assert im.count == (len(r.src) if isinstance(r.src, list) else 1)       # ONE album with the frame count it came with
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    _release(ims, clones)
    cf.release()


# eight albums of different sizes, none a whole multiple of the 16-pixel thumbnails, 2 to 5 frames
EIGHT = [(2, 21, 11), (3, 27, 19), (5, 33, 21), (4, 37, 23), (2, 43, 29), (3, 51, 33), (4, 57, 41), (5, 63, 47)]


def _eight(channels, cfg, **job):
    reqs = []
    for k, (frames, w, h) in enumerate(EIGHT):
        c = channels[k % len(channels)]
        if c == 4:
            reqs.append(GifReq(random_album(5400 + k, frames, w, h), bool(k & 1), cfg, **job))
        else:
            reqs.append(Req([noise_image(h, w, 3, 5500 + 10 * k + f) for f in range(frames)], cfg, **job))
    return reqs


def _frames_alone(reqs):
    """The same call with every album replaced by its frames as single images."""
    return [Req(a, r.cfg, **r.job) for r in reqs for a in r.src]


@pytest.mark.parametrize("what,channels,cfg,job,expected", [
    ("NN", [4], "plain", dict(resize="16,0", simple=1), 1),                            # (one launch per album before: 8)
    ("NN + gamma", [4], "plain", dict(resize="16,0", simple=1, filters=["gamma=1.4"]), 2),      # (16)
    ("AREA + overlay", [4, 3], "wm", dict(resize="16,0"), 2),                          # (8 or more)
])
def test_albums_cost_the_launches_of_their_frames(gpu, what, channels, cfg, job, expected):
    cf = _configs(gpu)
    reqs = _eight(channels, cfg, **job)
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    singles = _frames_alone(reqs)
    res1, launches1, ims1, _, _ = run_both(gpu, cf, singles, compare_loop=False)
    print("%s: %d albums %d launches; their %d frames alone %d launches" % (what, len(reqs), launches, len(singles), launches1))
    assert all(r == (0, 7) for r in res + res1)
    check_against_loop(res, ims, clones, loop)
    at = 0
    for im in ims:                                                   # the albums' frames are the single images' frames
        for f in im.frames():
            assert np.array_equal(f, ims1[at].numpy()), (what, at)
            at += 1
    assert launches == expected, (what, launches)
    assert launches == launches1, (what, launches, launches1)
    _release(ims, clones, ims1)
    cf.release()


@pytest.mark.parametrize("step", [STEP_RESIZE, STEP_WATERMARK])
def test_a_fault_point_cuts_one_album_once(gpu, step):
    """Three albums, the second entry into the step armed: the second ALBUM fails there (a point per request, not per frame),
    keeps what the per-request loop leaves it -- at RESIZE its own frames, byte for byte -- and the others are served."""
    cf = _configs(gpu)
    reqs = [GifReq(random_album(5600, 3, 37, 23), True, "wm", resize="20,0"),
            GifReq(random_album(5601, 4, 50, 30), False, "wm", resize="24,0"),
            Req([noise_image(21, 33, 3, 5610 + f) for f in range(2)], "wm", resize="18,0")]
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims]
    lib = gpu.lib
    try:
        assert lib.impgpu_fault_arm(step, 2) == 0
        res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        assert lib.impgpu_fault_arm(step, 2) == 0
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    finally:
        lib.impgpu_fault_arm(-1, 0)
    assert res == [(0, 7), (gpu.IMP_ERROR_DEVICE, step), (0, 7)], res
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims, skip=(1,))
    assert ims[1].count == 4
    if step == STEP_RESIZE:
        assert np.array_equal(_pixels(ims[1]), np.stack(reqs[1].src))
    _release(ims, clones)
    cf.release()


def test_a_gray_album_in_the_call_is_answered_as_by_run_ops(gpu):
    cf = _configs(gpu)
    reqs = [GifReq(random_album(5700, 2, 37, 23), False, "plain", resize="20,0", filters=["gamma=1.2"]),
            Req([noise_image(23, 37, 1, 5710 + f) for f in range(3)], "wm", resize="20,0", filters=["gamma=1.2"]),
            GifReq(random_album(5701, 3, 50, 30), True, "plain", resize="20,0", filters=["gamma=1.2"])]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    assert all(r == (0, 7) for r in res), res
    assert ims[1].count == 3 and ims[1].shape[2] == 3                # promoted, still one album of three
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    _release(ims, clones)
    cf.release()
