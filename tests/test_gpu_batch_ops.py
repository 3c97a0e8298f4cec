"""impgpu_batch_run_ops: RunJob's operator segment (bridge.c:574-656) for a queue of independent requests at once.

Every request must come out exactly as the per-request loop of impgpu_run_ops leaves it -- frame, code and step -- and as
the oracle chain makes it; the chains the mixed launch takes share one launch per channel count."""
import numpy as np
import pytest

from conftest import noise_image, smooth_image
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu

SIZES = [(480, 640), (600, 800), (768, 1024), (720, 1280), (768, 1366), (900, 1600), (1080, 1920), (1440, 2560),
         (2160, 3840)]
GRAVITIES = [(gx, gy) for gy in "tcb" for gx in "lcr"]


class Req:
    """One request: its source (an array, or a list of frames for an album), the name of its config, its job."""

    def __init__(self, src, cfg, **job):
        self.src, self.cfg, self.job = src, cfg, job

    def image(self, gpu):
        return gpu.Image.album(self.src) if isinstance(self.src, list) else gpu.Image(self.src)


def _pixels(im):
    return np.stack(im.frames()) if im.count > 1 else im.numpy()


class Configs:
    """Named configs (a location's settings), each with the oracle's view of its watermark."""

    def __init__(self, gpu):
        self.gpu, self.cfg, self.wm = gpu, {}, {}

    def add(self, name, overlay=None, wm=None, **kw):
        c = self.gpu.Config(**kw)
        if overlay is not None:
            assert c.prepare_watermark(overlay, *wm) == 0
        self.cfg[name] = c
        self.wm[name] = (overlay, wm, kw)

    def oracle(self, r, arr):
        overlay, wm, kw = self.wm[r.cfg]
        job = dict(r.job)
        flatten = job.pop("need_flatten", 0)
        if 0 < kw.get("max_filters", 5) < len(job.get("filters", ())):
            return 55, 0, None                          # refused while parsing (bridge.c:361-363), before any operator
        return oracle_chain(arr, overlay=overlay, wm=wm, flatten=flatten, allow=int(kw.get("allow_experiments", False)),
                            max_w=kw.get("max_w", 2000), max_h=kw.get("max_h", 2000), **job)

    def release(self):
        for c in self.cfg.values():
            c.release()


def run_both(gpu, cf, reqs, compare_loop=True):
    """The batch, and (on clones of the same frames) the per-request loop.  Returns (results, launches, images, loop)."""
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims] if compare_loop else None
    res, launches = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
    loop = None
    if compare_loop:
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    return res, launches, ims, clones, loop


def check_against_loop(res, ims, clones, loop):
    for i, (got, want) in enumerate(zip(res, loop)):
        assert got == want, (i, got, want)
        assert ims[i].shape == clones[i].shape and ims[i].count == clones[i].count, i
        assert np.array_equal(_pixels(ims[i]), _pixels(clones[i])), i


def check_against_oracle(cf, reqs, res, ims, skip=()):
    for i, r in enumerate(reqs):
        if i in skip:
            continue
        srcs = r.src if isinstance(r.src, list) else [r.src]
        outs = []
        for a in srcs:
            rc_o, step_o, want = cf.oracle(r, a)
            outs.append(want)
        assert res[i][0] == rc_o, (i, r.job, res[i], rc_o, step_o)
        if rc_o:
            assert res[i][1] == step_o, (i, r.job, res[i], step_o)
            continue
        assert res[i][1] == 7, (i, res[i])
        got = _pixels(ims[i])
        want = np.stack(outs) if isinstance(r.src, list) else outs[0]
        assert got.shape == want.shape and np.array_equal(got, want), (i, r.cfg, r.job)


def _release(*groups):
    for g in groups:
        for im in g or ():
            im.release()


def _sources():
    src = {}
    for k, (h, w) in enumerate(SIZES):
        src[(h, w, 3)] = noise_image(h, w, 3, 700 + k)
        src[(h, w, 4)] = smooth_image(h, w, 4, k)
    return src


def test_mixed_batch_matches_loop_and_oracle(gpu):
    cf = Configs(gpu)
    cf.add("plain", allow_experiments=True)
    for k, (gx, gy) in enumerate(GRAVITIES):
        ov = noise_image(24 + 7 * k, 40 + 11 * k, 4, 800 + k)
        cf.add("wm%d" % k, ov, (gx, gy, 3 * k - 10, 5 - 2 * k, 1 if k % 2 else 100), allow_experiments=True)
    cf.add("wide", noise_image(60, 300, 4, 820), ("c", "c", 0, 0, 60))                 # wider than every thumbnail: clipped
    cf.add("hang", noise_image(90, 120, 4, 821), ("r", "b", -70, -50, 100))            # pushed over the bottom right edge
    cf.add("small", max_w=100, max_h=100, max_filters=2)
    src = _sources()
    reqs = []
    for k, (h, w) in enumerate(SIZES):
        c = 3 + k % 2
        a = src[(h, w, c)]
        reqs.append(Req(a, "plain", crop="16,9", resize="224,0"))                                         # crop + resize
        reqs.append(Req(a, "plain", crop="%dpx,%dpx,%dpx,%dpx" % (w // 2, h // 2, 4 * k, 3 * k), resize="0,150"))
        reqs.append(Req(a, "wm%d" % k, resize="224,0"))                                                   # resize + watermark
        reqs.append(Req(src[(h, w, 7 - c)], "wm%d" % ((k + 4) % 9), resize="300,0"))
        reqs.append(Req(a, "wm%d" % k, resize="0,200", filters=["rotate=%d" % (90 * (1 + k % 3))]))     # + rotate + watermark
        reqs.append(Req(src[(h, w, 4)], "plain", resize="220,0", need_flatten=1))                        # BGRA + flatten
        reqs.append(Req(src[(h, w, 4)], "wm%d" % ((k + 2) % 9), crop="4,3,r,b", resize="180,0", filters=["rotate=270"],
                        need_flatten=1))                                                                   # all of it
    reqs.append(Req(src[(1080, 1920, 3)], "wide", resize="224,0", filters=["rotate=90"]))
    reqs.append(Req(src[(720, 1280, 4)], "hang", resize="230,0", need_flatten=1))
    reqs.append(Req(src[(768, 1366, 3)], "hang", crop="1,1", resize="101,0"))
    # ... and requests the mixed launch does not take, in the same call
    fall = len(reqs)
    reqs += [
        Req(noise_image(300, 400, 1, 830), "wm3", resize="120,0"),                          # gray
        Req(src[(480, 640, 3)], "plain", resize="900,700,up"),                               # CUBIC upscale
        Req(src[(600, 800, 4)], "wm1", resize="160,0", simple=1),                            # simple
        Req(src[(768, 1024, 3)], "wm2", resize="200,0", filters=["gamma=1.4"]),              # a pointwise filter
        Req(src[(720, 1280, 4)], "plain", resize="256,0", filters=["blur=1.5"]),             # blur
        Req([noise_image(240, 321, 3, 840 + i) for i in range(3)], "wm4", resize="100,0"),  # an album
        Req(src[(480, 640, 4)], "wm5", resize="320,240"),                                    # an exact 2x shrink
        Req(src[(480, 640, 3)], "plain", crop="0,0,320,240", resize="100,0"),                 # bad crop: 50 at step 3
        Req(src[(480, 640, 3)], "small", resize="500,500,up"),                                # over the limit: 54 at step 4
        Req(src[(600, 800, 3)], "plain", resize="100,0", filters=["nosuch=1"]),               # 52 at step 5
        Req(src[(600, 800, 4)], "small", resize="90,0", filters=["gamma=1"] * 3),             # 55 at step START
    ]
    assert len(reqs) >= 32
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert [r[:2] for r in res[-4:]] == [(50, 3), (54, 4), (52, 5), (55, 0)]
    assert all(r[0] == 0 for r in res[:fall])
    assert launches < len(reqs)
    _release(ims, clones)
    cf.release()


def _thumbs(n, channels):
    """n sources of n different sizes, none of them an integer multiple of the thumbnail's."""
    out = []
    for k in range(n):
        h, w = 401 + 61 * k, 617 + 97 * k
        c = channels[k % len(channels)]
        out.append(noise_image(h, w, c, 900 + k) if c == 3 else smooth_image(h, w, c, k))
    return out


def test_watermarked_thumbnails_share_one_launch(gpu):
    cf = Configs(gpu)
    cf.add("wm", noise_image(32, 80, 4, 950), ("r", "b", 8, 8, 70))
    reqs = [Req(a, "wm", resize="224,0") for a in _thumbs(16, [3])]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 1, launches          # the per-request loop: a resize and a blend each, 32 launches
    _release(ims, clones)
    reqs = [Req(a, "wm", resize="224,0", filters=["rotate=90"] if k % 3 == 0 else [], need_flatten=k % 2)
            for k, a in enumerate(_thumbs(16, [3, 4]))]
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert launches == 2, launches          # one per channel count
    _release(ims, clones)
    cf.release()


@pytest.mark.parametrize("step", [6, 4])
def test_fault_injector_fails_the_same_request(gpu, step):
    cf = Configs(gpu)
    cf.add("wm", noise_image(32, 80, 4, 960), ("l", "t", 2, 2, 100), allow_experiments=True)
    src = _thumbs(10, [3, 4])
    # the third request rides the mixed launch; the second goes through impgpu_run_ops and enters the same steps before it
    jobs = [dict(resize="224,0"), dict(resize="200,0", filters=["gamma=1.3"]), dict(resize="224,0", filters=["rotate=90"], need_flatten=1),
            dict(resize="224,0", need_flatten=1), dict(crop="16,9", resize="180,0", filters=["rotate=180"], need_flatten=1)]
    reqs = [Req(a, "wm", **jobs[k % len(jobs)]) for k, a in enumerate(src)]
    lib = gpu.lib
    ims = [r.image(gpu) for r in reqs]
    clones = [im.clone() for im in ims]
    try:
        assert lib.impgpu_fault_arm(step, 3) == 0
        res, _ = gpu.batch_run_ops(ims, [cf.cfg[r.cfg] for r in reqs], [r.job for r in reqs])
        assert lib.impgpu_fault_arm(step, 3) == 0
        loop = [gpu.run_ops(cl, cf.cfg[r.cfg], **r.job) for cl, r in zip(clones, reqs)]
    finally:
        lib.impgpu_fault_arm(-1, 0)
    failed = [i for i, r in enumerate(res) if r[0] != 0]
    assert failed == [2], res                                  # every request enters both steps: the third one fails
    assert res[2] == (gpu.IMP_ERROR_DEVICE, step)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims, skip=(2,))
    _release(ims, clones)
    cf.release()


def test_large_batch(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(40, 96, 4, 970), ("r", "b", 10, 10, 55))
    big = [noise_image(2160, 3840, 3, 971), smooth_image(2160, 3840, 4, 3)]
    src = _thumbs(24, [3, 4])
    reqs = []
    for k in range(256):
        if k % 32 == 0:
            a = big[(k // 32) % 2]
            reqs.append(Req(a, "wm", resize="%d,0" % (214 + k // 32), filters=["rotate=90"] if k % 64 else []))   # 17.9x .. 17.4x
            continue
        a = src[k % len(src)]
        job = [dict(resize="160,0"), dict(crop="16,9", resize="128,0"), dict(resize="0,96", filters=["rotate=270"]),
               dict(resize="200,0", need_flatten=1)][k % 4]
        reqs.append(Req(a, "wm" if k % 3 else "plain", **job))
    res, launches, ims, _, _ = run_both(gpu, cf, reqs, compare_loop=False)
    check_against_oracle(cf, reqs, res, ims)
    assert launches < 16, launches         # the loop: one to three launches for each of 256 requests
    _release(ims)
    cf.release()
