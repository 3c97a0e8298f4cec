"""The broker runs every request of a batch through impgpu_batch_run_ops: crops, turns, watermarks and flattens of different
workers share launches.  Each answer must still be the bytes the oracle makes for that request alone."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle_lib as orc
from conftest import ROOT, noise_image, smooth_image
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_CLIENTS = 8
ROUNDS = 4


def _photo(h, w, seed):
    from ngx_http_imgproc_amd.workloads import photo_like
    return photo_like(h, w, seed)[:, :, ::-1].copy()          # B,G,R


@pytest.fixture(scope="module")
def scaling():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "ngx_http_imgproc_amd", "build.py")], stdout=subprocess.DEVNULL)
    import worker_scaling
    return worker_scaling


def test_chains_of_many_workers_share_launches_and_match_the_oracle(scaling):
    from ngx_http_imgproc_amd import broker as B
    from ngx_http_imgproc_amd._lib import CConfig

    ov = noise_image(28, 72, 4, 61)
    wm = ("r", "b", 6, 4, 70)
    cfg_wm = CConfig(2000, 2000, 5, 0, wm[4], wm[0].encode(), wm[1].encode(), wm[2], wm[3], None)
    cases = []                                                 # (request kwargs, uses the watermark, the oracle's answer)
    for k, (h, w) in enumerate([(480, 640), (720, 1280), (1080, 1920), (600, 800)]):
        rc, blob = orc.jpeg_encode(_photo(h, w, 20 + k), 90)
        assert rc == 0
        rc, frame = orc.jpeg_decode(blob)
        assert rc == 0
        # crop + resize, answered as a JPEG file
        rc, _, small = oracle_chain(frame, crop="320px,240px,0px,0px", resize="224,0")
        rc_e, want = orc.jpeg_encode(small, 86)
        assert rc == rc_e == 0
        cases.append((dict(blob=blob, crop="320px,240px,0px,0px", resize="224,0", out=B.OUT_JPEG), False, want))
        # crop + resize + the location's watermark, as pixels
        rc, _, want = oracle_chain(frame, crop="16,9", resize="224,0", overlay=ov, wm=wm)
        assert rc == 0
        cases.append((dict(blob=blob, crop="16,9", resize="224,0", out=B.OUT_FRAME), True, want))
        # resize + turn + watermark
        rc, _, want = oracle_chain(frame, resize="960,540", filters=["rotate=90"], overlay=ov, wm=wm)
        assert rc == 0
        cases.append((dict(blob=blob, resize="960,540", filters=["rotate=90"], out=B.OUT_FRAME), True, want))
        # a BGRA frame for an encoder without alpha
        rgba = smooth_image(h // 2 + 3 * k, w // 2 + 5 * k, 4, k)
        rc, _, want = oracle_chain(rgba, resize="200,0", flatten=1)
        assert rc == 0
        cases.append((dict(frame=rgba, resize="200,0", need_flatten=1, out=B.OUT_FRAME), False, want))

    name = "/impgpu-chains-%d" % os.getpid()
    p = scaling.start_broker(name, threads=2, gather_us=3000, slots=16, extra=["--slot-mb", "24"])
    failures, batch_sizes = [], []
    try:
        barrier = threading.Barrier(N_CLIENTS)

        def client(t):
            c = B.Client(name)
            try:
                wid = c.prepare_watermark(ov)                  # the location's overlay, registered by every worker
                barrier.wait(timeout=120)
                for r in range(ROUNDS):
                    for j in range(len(cases)):
                        kw, with_wm, want = cases[(j + 3 * t + r) % len(cases)]
                        extra = dict(config=cfg_wm, watermark_id=wid) if with_wm else {}
                        rc, code, step, got, a = c.run(**kw, **extra)
                        batch_sizes.append(a.batch_size)
                        if rc or code:
                            failures.append((t, kw.get("crop"), kw.get("resize"), rc, code, step, B.Client.last_error()))
                        elif isinstance(want, bytes):
                            if got != want:
                                failures.append((t, kw.get("crop"), kw.get("resize"), "JPEG differs"))
                        elif got.shape != want.shape or not np.array_equal(got, want):
                            failures.append((t, kw.get("crop"), kw.get("resize"), kw.get("filters"), "frame differs"))
            except Exception as e:                             # (reported below, in the test's thread)
                failures.append((t, repr(e)))
            finally:
                c.close()

        threads = [threading.Thread(target=client, args=(t,)) for t in range(N_CLIENTS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=600)
        assert not any(th.is_alive() for th in threads)
    finally:
        err = scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    assert not os.path.exists("/dev/shm" + name)              # a clean stop leaves no segment behind
    assert not failures, failures[:8]
    assert len(batch_sizes) == N_CLIENTS * ROUNDS * len(cases)
    assert max(batch_sizes) > 1, batch_sizes                    # requests of different workers rode one batch
