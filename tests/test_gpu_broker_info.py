"""The broker answers the json exits (Info(), bridge.c:283-300) and the text exits (ASCII(), bridge.c:668-676) of a batch
with one impgpu_batch_calc_perceived_brightness / impgpu_batch_ascii each instead of a call and a wait per request.  Every
answer must still be what the oracle gives for that request alone; a lone request keeps the lone call."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle_lib as orc
from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_CLIENTS = 8
SIZES = [(480, 640), (720, 1280), (1080, 1920), (600, 800), (300, 256), (1200, 1600), (768, 1024), (360, 480)]
JSON_WIDTHS = [100, 224, 160, 320, 96, 400, 257, 64]          # resize=<w>,0 per client
TEXT_WIDTHS = [60, 72, 48, 80, 33, 100, 64, 20]


def _photo(h, w, seed):
    from ngx_http_imgproc_amd.workloads import photo_like
    return photo_like(h, w, seed)[:, :, ::-1].copy()          # B,G,R


@pytest.fixture(scope="module")
def scaling():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "ngx_http_imgproc_amd", "build.py")], stdout=subprocess.DEVNULL)
    import worker_scaling
    return worker_scaling


@pytest.fixture
def broker(scaling):
    """As tests/test_gpu_broker.py's, with a gather window long enough for clients released together to meet."""
    name = "/impgpu-test-info-%d" % os.getpid()
    p = scaling.start_broker(name, threads=2, gather_us=20000, slots=16, extra=["--slot-mb", "24"])
    yield name, p
    err = scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    assert not os.path.exists("/dev/shm" + name)              # a clean stop leaves no segment behind


def _cases():
    """Per client: its file, and per wave the request and the oracle's answer to it."""
    from ngx_http_imgproc_amd import broker as B

    out = []
    for t, (h, w) in enumerate(SIZES):
        rc, blob = orc.jpeg_encode(_photo(h, w, 40 + t), 90)
        assert rc == 0
        rc, frame = orc.jpeg_decode(blob)
        assert rc == 0

        def json_case(width):
            rc, small = orc.resize(frame, "%d,0" % width)
            assert rc == 0
            return dict(blob=blob, resize="%d,0" % width, out=B.OUT_INFO), ("json", np.float32(orc.brightness(small)), small.shape)

        def text_case(width, args):
            rc, small = orc.resize(frame, "%d,0" % width)
            assert rc == 0
            return dict(blob=blob, resize="%d,0" % width, out=B.OUT_ASCII, ascii_args=args), ("text", orc.ascii_art(small, args or ""), small.shape)

        def jpeg_case(width):
            rc, small = orc.resize(frame, "%d,0" % width)
            rc_e, want = orc.jpeg_encode(small, 86)
            assert rc == rc_e == 0
            return dict(blob=blob, resize="%d,0" % width, out=B.OUT_JPEG, quality=86), ("jpeg", want, small.shape)

        waves = [json_case(JSON_WIDTHS[t]), text_case(TEXT_WIDTHS[t], ["", "wide", None][t % 3])]
        waves.append([json_case(JSON_WIDTHS[(t + 3) % 8]), text_case(TEXT_WIDTHS[(t + 5) % 8], "wide" if t % 2 else ""), jpeg_case(224 - 8 * t)][t % 3])
        out.append(waves)
    return out


def _check(kind_want, rc, code, step, got, a):
    kind, want, shape = kind_want
    if rc or code:
        return "rc %d code %d step %d" % (rc, code, step)
    if (a.width, a.height) != (shape[1], shape[0]):
        return "%s: geometry %dx%d, not %dx%d" % (kind, a.width, a.height, shape[1], shape[0])
    if kind == "json":
        return None if np.float32(a.brightness) == want else "json: brightness %r, not %r" % (a.brightness, want)
    return None if got == want else "%s differs" % kind


def test_json_and_text_requests_of_many_workers_meet_and_match_the_oracle(broker):
    from ngx_http_imgproc_amd import broker as B

    name, _ = broker
    cases = _cases()
    failures = []
    batch_sizes = [[], [], []]
    barrier = threading.Barrier(N_CLIENTS)

    def client(t):
        c = B.Client(name)
        try:
            for wave in range(3):
                kw, want = cases[t][wave]
                barrier.wait(timeout=120)                      # all eight submit at the same moment
                rc, code, step, got, a = c.run(**kw)
                batch_sizes[wave].append(a.batch_size)
                bad = _check(want, rc, code, step, got, a)
                if bad:
                    failures.append((t, wave, kw["resize"], bad, B.Client.last_error()))
        except Exception as e:                                 # (reported below, in the test's thread)
            failures.append((t, repr(e)))
            barrier.abort()
        finally:
            c.close()

    threads = [threading.Thread(target=client, args=(t,)) for t in range(N_CLIENTS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    assert not any(th.is_alive() for th in threads)
    assert not failures, failures[:8]
    print("\nbatch sizes per wave:", batch_sizes)
    for wave in range(3):
        assert len(batch_sizes[wave]) == N_CLIENTS
        assert max(batch_sizes[wave]) > 1, (wave, batch_sizes[wave])   # the requests did meet


def test_a_lone_json_and_a_lone_text_request_answer_as_before(broker):
    """What test_every_kind_of_request_and_answer asks of the two exits -- and to the bit."""
    from ngx_http_imgproc_amd import broker as B

    name, _ = broker
    c = B.Client(name)
    rc, blob = orc.jpeg_encode(_photo(480, 640, 11), 90)
    rc, frame = orc.jpeg_decode(blob)
    rc, code, step, got, a = c.run(blob=blob, resize="100,0", out=B.OUT_INFO)
    rc_o, small = orc.resize(frame, "100,0")
    assert (rc, code) == (0, 0) and (a.width, a.height) == (small.shape[1], small.shape[0])
    assert abs(a.brightness - orc.brightness(small)) < 1e-6
    assert np.float32(a.brightness) == np.float32(orc.brightness(small))
    assert a.batch_size == 1
    rc, code, step, got, a = c.run(blob=blob, resize="60,0", out=B.OUT_ASCII, ascii_args="")
    rc_o, small = orc.resize(frame, "60,0")
    assert (rc, code) == (0, 0) and got == orc.ascii_art(small, "") and a.batch_size == 1
    # a failing chain in front of the exit keeps its code and step
    rc, code, step, got, a = c.run(blob=blob, filters=["nosuch=1"], out=B.OUT_INFO)
    assert rc == 0 and code == 52 and step == 5
    c.close()
