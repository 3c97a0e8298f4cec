"""GIF requests of one batch through a real broker: their albums ride the batch's shared operator launches, their FreeImage
answers leave through ONE impgpu_batch_download_fi and their frame answers through ONE impgpu_batch_album_download, next to the
JPEG requests of the same gather window.  Every answer equals the answer the same request gets alone, and the oracle's."""
import os
import sys
import threading

import numpy as np
import pytest

import oracle_lib as orc
from conftest import ROOT, noise_image
from test_gif import random_album
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def served():
    """A broker as tests/test_gpu_broker_album.py starts it: slots of 2 MB, a gather window so that requests submitted together
    ride together.  It must stop with exit status 0 after everything the test sent it."""
    import subprocess
    subprocess.check_call([sys.executable, os.path.join(ROOT, "ngx_http_imgproc_amd", "build.py")], stdout=subprocess.DEVNULL)
    import worker_scaling
    from ngx_http_imgproc_amd import broker as B
    name = "/impgpu-test-album-batch-%d" % os.getpid()
    p = worker_scaling.start_broker(name, threads=2, gather_us=20000, slots=12, extra=["--slot-mb", "2"])
    yield B, name, p
    err = worker_scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    assert not os.path.exists("/dev/shm" + name)


def _same(got, want):
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
    return got.shape == want.shape and np.array_equal(got, want)


def test_gif_answers_of_one_batch_leave_together(served):
    B, name, p = served
    # six GIFs answered as FreeImage bitmaps (32 and 24 bits mixed), two answered frame by frame, two JPEG files
    albums = [(random_album(7000 + i, 2 + i % 4, 20 + 7 * i, 9 + 5 * i), bool(i & 1)) for i in range(8)]
    blobs = [orc.jpeg_encode(noise_image(40 + 8 * i, 56, 3, 7100 + i), 90)[1] for i in range(2)]
    job = dict(resize="16,0", simple=1)
    asks = [dict(gif_pages=pg, destructive=d, out=B.OUT_FI, quality=32 if i % 3 else 24, **job) for i, (pg, d) in enumerate(albums[:6])] + \
           [dict(gif_pages=pg, destructive=d, out=B.OUT_FRAME, **job) for pg, d in albums[6:]] + \
           [dict(blob=b, resize="24,0", out=B.OUT_FRAME) for b in blobs]
    # the oracle's answers
    want = []
    for ask, (pg, d) in zip(asks, albums):
        rc_o, frames = orc.gif_compose(pg, d)
        assert rc_o == 0
        small = []
        for f in frames:
            rc_o, _, s = oracle_chain(f, **job)
            assert rc_o == 0
            small.append(orc.ipl_to_fi(s, ask["quality"]) if ask["out"] == B.OUT_FI else s)
        want.append(small)
    for b in blobs:
        rc_o, _, s = oracle_chain(orc.jpeg_decode(b)[1], resize="24,0")
        assert rc_o == 0
        want.append(s)

    def check(results):
        for i, (ask, r, w) in enumerate(zip(asks, results, want)):
            assert r[:2] == (0, 0), (i, r[:3])
            if ask["out"] == B.OUT_FI:
                rowbytes = r[4].width * ask["quality"] // 8
                assert r[4].frames == len(w) and r[4].channels == ask["quality"] // 8
                assert _same([g[:, :rowbytes] for g in r[3]], [x[:, :rowbytes] for x in w]), i
            else:
                assert _same(r[3], w), i

    clients = [B.Client(name) for _ in asks]
    alone = [c.run(**ask) for c, ask in zip(clients, asks)]
    check(alone)
    together = [None] * len(asks)
    gate = threading.Barrier(len(asks))

    def ask_one(i):
        gate.wait()
        together[i] = clients[i].run(**asks[i])
    threads = [threading.Thread(target=ask_one, args=(i,)) for i in range(len(asks))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    check(together)
    for lone, r in zip(alone, together):
        assert _same(r[3], lone[3])
    assert max(r[4].batch_size for r in together) > 1, [r[4].batch_size for r in together]
    assert p.poll() is None
    for c in clients:
        c.close()
