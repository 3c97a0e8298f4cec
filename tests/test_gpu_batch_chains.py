"""impgpu_batch_run_ops on chains with filters: [crop ->] resize -> any filters -> [watermark] -> [flatten] in shared launches.

The resizes go first, then round k launches the k-th segment of every chain (a pointwise run with the tail, a blur, a flip or
a turn), one launch per kind and channel count.  Every request must still come out exactly as the per-request loop of
impgpu_run_ops leaves it -- frame, code and step -- and, where the oracle is exact, as the oracle chain makes it."""
import numpy as np
import pytest

from conftest import noise_image, smooth_image
from test_gpu_batch_ops import SIZES, Configs, Req, check_against_loop, check_against_oracle, run_both
from test_gpu_broker_chains import _photo, scaling  # noqa: F401  (the broker fixture)
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu

# 30 pointwise filters: more stages and table bytes than one k_pixel_program launch holds, so the run is cut in two
LONG_CHAIN = ["modulate=%d,110,95" % (7 * k % 180) if k % 3 == 0 else ("gamma=1.%d" % (k % 9 + 1) if k % 3 == 1 else "gradmap=102030,c0b0a0")
              for k in range(30)]


def _release(*groups):
    for g in groups:
        for im in g or ():
            im.release()


def _sources():
    src = {}
    for k, (h, w) in enumerate(SIZES):
        src[(h, w, 3)] = noise_image(h, w, 3, 1700 + k)
        src[(h, w, 4)] = smooth_image(h, w, 4, 30 + k)
    return src


def _configs(gpu):
    cf = Configs(gpu)
    cf.add("plain")
    cf.add("exp", allow_experiments=True)
    cf.add("wm", noise_image(30, 76, 4, 1750), ("r", "b", 6, 4, 70), allow_experiments=True)
    cf.add("wm3", noise_image(26, 50, 3, 1751), ("l", "t", 3, 2, 45))                # a 3-channel overlay
    cf.add("long", noise_image(20, 40, 4, 1752), ("c", "c", 0, 0, 100), max_filters=40)
    return cf


# (config, job) kinds: every one a chain the fused resize launch alone does not take
CHAINS = [
    ("wm", dict(resize="224,0", filters=["gamma=1.4"])),
    ("exp", dict(resize="200,0", filters=["gotham=1"])),
    ("wm3", dict(crop="16,9", resize="180,0", filters=["modulate=30,120,80", "contrast=1.5"])),
    ("wm", dict(resize="224,0", filters=["blur=0.5"])),                                   # kernel size 5: k_blur_fused4
    ("plain", dict(resize="240,0", filters=["blur=1.5"])),                                # k_blur_mfma_fused
    ("wm3", dict(resize="220,0", filters=["blur=3"])),
    ("wm", dict(resize="256,0", filters=["flip=10", "blur=2", "colorize=ff8000,0.3"])),
    ("wm", dict(resize="224,0", filters=["rotate=90", "gamma=1.7"])),                      # the turn rides the AREA stores
    ("plain", dict(resize="210,0", filters=["blur=1", "flip=01"])),                       # two barriers in a row
    ("wm", dict(resize="0,160", filters=["rotate=270", "flip=11", "contrast=0.7"])),
]


def test_filtered_batch_matches_loop_and_oracle(gpu):
    cf = _configs(gpu)
    src = _sources()
    reqs, vignette = [], []
    for k, (h, w) in enumerate(SIZES):
        for j, (cfg, job) in enumerate(CHAINS[k % 2::2] + [CHAINS[(k + 3) % len(CHAINS)]]):
            c = 3 + (k + j) % 2
            job = dict(job)
            if c == 4 and j % 2:
                job["need_flatten"] = 1
            reqs.append(Req(src[(h, w, c)], cfg, **job))
    a3, a4 = src[(480, 640, 3)], src[(600, 800, 4)]
    reqs += [
        Req(a4, "wm", resize="0,150", filters=["blur=12"], need_flatten=1),                  # a lone blur form inside its round
        Req(a3, "plain", resize="200,0", filters=["blur=12", "gamma=1.2"]),
        Req(a3, "exp", resize="900,700,up", filters=["gamma=0.8"]),                          # CUBIC enlargement
        Req(src[(480, 640, 4)], "exp", resize="700,600,up", filters=["vignette=0.8,0.6"]),
        Req(a4, "wm", resize="1000,0,up", filters=["rotate=180"], need_flatten=1),           # a half turn, not on the resize
        Req(a3, "long", resize="190,0", filters=LONG_CHAIN),                                  # one run in two launches
        Req(a4, "long", crop="4,3,r,b", resize="150,0", filters=["blur=2"] + LONG_CHAIN[:20], need_flatten=1),
        Req(a3, "plain", resize="100,0", filters=["blur=2", "nosuch=1"]),                    # 52 at step 5
        Req(a4, "wm", resize="90,0", filters=["gamma=1"] * 6),                               # 55 at step START
        Req(a3, "wm", resize="200,0", simple=1, filters=["gamma=1.3", "flip=10"]),           # NN
    ]
    vignette.append(len(reqs) - 7)
    assert len(reqs) >= 64
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims, skip=vignette)
    for i in vignette:                                      # the reference's vignette is a double cos: within one
        rc, _, want = cf.oracle(reqs[i], reqs[i].src)
        assert rc == 0 and res[i][0] == 0
        assert np.abs(ims[i].numpy().astype(int) - want.astype(int)).max() <= 1
    assert [r[:2] for r in res[-3:-1]] == [(52, 5), (55, 0)]
    assert all(r[0] == 0 for r in res[:-3]) and res[-1][0] == 0
    _release(ims, clones)
    cf.release()


def _kinds(k):
    """`k` requests of each chain kind, on sources of different sizes that are no integer multiple of the thumbnails."""
    reqs = []
    for rep in range(k):
        for j, (cfg, job) in enumerate(CHAINS):
            for c in (3, 4):
                h, w = 401 + 37 * j + 5 * rep + c, 617 + 53 * j + 7 * rep
                a = noise_image(h, w, 3, 1800 + 10 * j + rep) if c == 3 else smooth_image(h, w, 4, 10 * j + rep)
                reqs.append(Req(a, cfg, **job))
    return reqs


def test_launches_do_not_grow_with_the_count(gpu):
    cf = _configs(gpu)
    counts = []
    for k in (1, 4):
        reqs = _kinds(k)
        res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
        check_against_loop(res, ims, clones, loop)
        check_against_oracle(cf, reqs, res, ims)
        counts.append(launches)
        _release(ims, clones)
    cf.release()
    # Every kind comes in both channel counts, so k = 1 and k = 4 make the same groups.  The longest chain has three segments
    # after its resize: four rounds.  Per channel count the resize round launches at most two kernels (bare resizes, and
    # resizes with the turn on their stores) and every later round at most five: one pointwise / tail launch, one flip /
    # turn launch and one per blur form (k_blur_fused4, k_blur_mfma_fused with two or three byte planes).  Bound:
    # 2 x (2 + 3 x 5) = 34.  The per-request loop enqueues two to four launches per request: over 160 for the 80 of k = 4.
    assert counts[0] == counts[1], counts
    assert counts[1] <= 34, counts


# every way a cut can land: a tail with a pointwise run; a blur, then a tail; a turn on the resize's stores, then a flip; a lone
# turn whose launch carries the overlay; a blur whose tail is the watermark alone; a watermark and a flatten folded onto the
# resize's stores; a turn on the stores, then a pointwise tail
FAULT_JOBS = [dict(crop="16,9", resize="224,0", filters=["gamma=1.3"], need_flatten=1),
              dict(resize="200,0", filters=["blur=1.5", "contrast=1.2"]),
              dict(crop="4,3,c,c", resize="180,0", filters=["rotate=90", "flip=10"], need_flatten=1),
              dict(resize="210,0", filters=["rotate=270"], need_flatten=1),
              dict(resize="190,0", filters=["blur=2"]),
              dict(crop="1,1", resize="170,0", need_flatten=1),
              dict(crop="3,2", resize="0,150", filters=["rotate=90", "gamma=1.6"])]
FAULT_CHANNELS = [4, 3, 4, 4, 3, 4, 3]


def _fault_batch():
    """Two requests of every kind of FAULT_JOBS, request k of kind k mod 7."""
    reqs = []
    for k in range(2 * len(FAULT_JOBS)):
        j = k % len(FAULT_JOBS)
        h, w = 401 + 41 * k, 617 + 59 * k
        a = noise_image(h, w, 3, 1900 + k) if FAULT_CHANNELS[j] == 3 else smooth_image(h, w, 4, 60 + k)
        reqs.append(Req(a, "wm", **FAULT_JOBS[j]))
    return reqs


@pytest.mark.parametrize("step,kind", [(st, j) for st in (3, 4, 5, 6) for j in range(len(FAULT_JOBS))
                                       if (st != 3 or "crop" in FAULT_JOBS[j]) and (st != 5 or FAULT_JOBS[j].get("filters"))])
def test_fault_points_cut_the_same_request(gpu, step, kind):
    cf = _configs(gpu)
    reqs = _fault_batch()
    # the requests that enter this step, in order: CROP with a crop, FILTERING with filters, RESIZE and WATERMARK all of them
    entering = [i for i, r in enumerate(reqs) if (step != 3 or "crop" in r.job) and (step != 5 or r.job.get("filters"))]
    target = kind + len(FAULT_JOBS) * (kind % 2)             # the first or the second request of the kind
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
    assert res[failed[0]] == (gpu.IMP_ERROR_DEVICE, step)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims, skip=failed)
    _release(ims, clones)
    cf.release()


def test_broker_batches_filtered_requests(scaling):  # noqa: F811
    import os
    import threading

    import oracle_lib as orc
    from ngx_http_imgproc_amd import broker as B
    from ngx_http_imgproc_amd._lib import CConfig

    ov = noise_image(28, 72, 4, 1961)
    wm = ("r", "b", 6, 4, 70)
    cfg_wm = CConfig(2000, 2000, 5, 0, wm[4], wm[0].encode(), wm[1].encode(), wm[2], wm[3], None)
    chains = [["gamma=1.4"], ["blur=2"], ["flip=01", "blur=1.5"], ["modulate=30,120,80", "contrast=1.5"]]
    cases = []
    for k, (h, w) in enumerate([(480, 640), (720, 1280), (600, 800)]):
        rc, blob = orc.jpeg_encode(_photo(h, w, 40 + k), 90)
        assert rc == 0
        rc, frame = orc.jpeg_decode(blob)
        assert rc == 0
        for filters in chains:
            rc, _, small = oracle_chain(frame, resize="224,0", filters=filters, overlay=ov, wm=wm)
            rc_e, want = orc.jpeg_encode(small, 86)
            assert rc == rc_e == 0
            cases.append((dict(blob=blob, resize="224,0", filters=filters, out=B.OUT_JPEG), want))
    n_clients, rounds = 6, 2
    name = "/impgpu-filtered-%d" % os.getpid()
    p = scaling.start_broker(name, threads=2, gather_us=3000, slots=16, extra=["--slot-mb", "24"])
    failures, batch_sizes = [], []
    try:
        barrier = threading.Barrier(n_clients)

        def client(t):
            c = B.Client(name)
            try:
                wid = c.prepare_watermark(ov)
                barrier.wait(timeout=120)
                for r in range(rounds):
                    for j in range(len(cases)):
                        kw, want = cases[(j + 5 * t + r) % len(cases)]
                        rc, code, step, got, a = c.run(**kw, config=cfg_wm, watermark_id=wid)
                        batch_sizes.append(a.batch_size)
                        if rc or code:
                            failures.append((t, kw["filters"], rc, code, step, B.Client.last_error()))
                        elif got != want:
                            failures.append((t, kw["filters"], "JPEG differs"))
            except Exception as e:                             # (reported below, in the test's thread)
                failures.append((t, repr(e)))
            finally:
                c.close()

        threads = [threading.Thread(target=client, args=(t,)) for t in range(n_clients)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=600)
        assert not any(th.is_alive() for th in threads)
    finally:
        err = scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    assert not failures, failures[:8]
    assert len(batch_sizes) == n_clients * rounds * len(cases)
    assert max(batch_sizes) > 1, batch_sizes
