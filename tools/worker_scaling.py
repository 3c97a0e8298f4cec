"""N IMP worker PROCESSES on one GPU, one request at a time each (docs/02 - Configuration.md:18 worker_processes; module.c:298
RunJob synchronous): JPEG in -> resize=224,0 -> JPEG out, the mixed-size pool of bench.py --stream --jpeg.
    direct : every worker links libimpgpu.so and owns a device context (tests/c/worker_harness.c direct)
    broker : one impgpu_broker owns the device, workers are plain C clients of its shared-memory segment
Every size is warm before the clock; each point runs SECONDS (default 3).  One JSON line per point.
    python tools/worker_scaling.py direct 1 2 4 6
    python tools/worker_scaling.py broker 1 2 4 8 16 32 [--threads 2] [--gather-us 0] [--seconds 3]
(the GPU box allows at most 6 processes on the card: direct stops at 6, the broker is ONE such process however many workers)"""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HARNESS = os.path.join(ROOT, "tests", "c", "_build", "worker_harness")
# Other requests than resize=224,0 (broker only): --query takes a query string (impgpu_parse_request), --watermark the location's
# placement gx,gy,ox,oy,opacity of a fixed 96 x 32 BGRA overlay; the workers are then tools/request_worker.c.  --check writes the
# oracle's answers for the pool and that request first, and every answer is compared with them.  --pool png sends the same
# files as PNG uploads (the broker decodes a batch's PNG files in one impgpu_batch_decode_png call).
#     python tools/worker_scaling.py broker 1 8 16 32 --query "crop=16,9&resize=224,0" --watermark r,b,6,4,70 --check
#     python tools/worker_scaling.py broker 16 32 --pool png --check
REQUEST_WORKER = os.path.join(ROOT, "tools", "_build", "request_worker")
BROKER = os.path.join(ROOT, "ngx_http_imgproc_amd", "impgpu_broker")


def write_pool(path, blobs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for b in blobs:
            f.write(struct.pack("<I", len(b)))
            f.write(b)


def make_pool(path, n_files=64):
    if os.path.exists(path):
        return
    import bench

    write_pool(path, [b for _, _, b in bench.jpeg_pool(n_files)])


def make_png_pool(path, n_files=64):
    """The same files as make_pool's, as PNG (RGB, Pillow's default level): PNG uploads through the broker."""
    if os.path.exists(path):
        return
    import io

    import bench
    from PIL import Image

    blobs = []
    for _, _, jpeg in bench.jpeg_pool(n_files):
        b = io.BytesIO()
        Image.open(io.BytesIO(jpeg)).convert("RGB").save(b, "PNG")
        blobs.append(b.getvalue())
    write_pool(path, blobs)


def start_broker(name, threads, gather_us, slots=64, extra=(), env=None):
    d = tempfile.mkdtemp(prefix="impb_")
    ready = os.path.join(d, "ready")
    p = subprocess.Popen([BROKER, "--name", name, "--threads", str(threads), "--gather-us", str(gather_us), "--slots", str(slots),
                          "--ready-file", ready] + list(extra), stderr=subprocess.PIPE, text=True, env=dict(os.environ, **(env or {})))
    t_end = time.time() + 180
    while not os.path.exists(ready):
        if p.poll() is not None or time.time() > t_end:
            raise SystemExit("broker did not start: %s" % p.stderr.read()[-800:])
        time.sleep(0.01)
    shutil.rmtree(d, ignore_errors=True)
    return p


def stop_broker(p):
    p.terminate()
    try:
        _, err = p.communicate(timeout=60)
    except subprocess.TimeoutExpired:
        p.kill()
        _, err = p.communicate()
    return err


def build_request_worker():
    src = [os.path.join(ROOT, "tools", "request_worker.c"), os.path.join(ROOT, "glue", "imp_gpu_client.c")]
    deps = src + [os.path.join(ROOT, "include", "impgpu.h"), os.path.join(ROOT, "include", "impgpu_broker.h")]
    if os.path.exists(REQUEST_WORKER) and all(os.path.getmtime(f) <= os.path.getmtime(REQUEST_WORKER) for f in deps):
        return
    os.makedirs(os.path.dirname(REQUEST_WORKER), exist_ok=True)
    lib = os.path.join(ROOT, "ngx_http_imgproc_amd")
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include")] + src +
                          ["-o", REQUEST_WORKER, "-L", lib, "-limpgpu", "-lm", "-lrt", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"])


def overlay_frame():
    """The --watermark overlay: 32 x 96 BGRA, fixed noise."""
    import numpy as np

    return np.random.Generator(np.random.PCG64(0x1A4D0096)).integers(0, 256, size=(32, 96, 4), dtype=np.uint8)


def write_overlay(path):
    ov = overlay_frame()
    with open(path, "wb") as f:
        f.write(struct.pack("<III", ov.shape[1], ov.shape[0], ov.shape[2]))
        f.write(ov.tobytes())


def oracle_answers(pool, query, placement, path):
    """The file the reference writes for every pool file under `query` (and the --watermark placement), quality 86 unless
    the query names one: the CPU oracle's decode -> RunJob's operators -> encode."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as orc
    import ngx_http_imgproc_amd as imp

    req = imp.Request("/pool.jpg?" + query, "jpg", imp.Config())
    assert req.code == 0, (query, req.code)
    quality = int(req.quality) if req.quality else 86
    with open(pool, "rb") as f:
        data = f.read()
    n, at, blobs = struct.unpack_from("<I", data, 0)[0], 4, []
    for _ in range(n):
        sz = struct.unpack_from("<I", data, at)[0]
        blobs.append(data[at + 4:at + 4 + sz])
        at += 4 + sz
    answers = []
    for b in blobs:
        rc, cur = orc.png_decode(b) if b[:8] == b"\x89PNG\r\n\x1a\n" else orc.jpeg_decode(b)
        assert rc == 0
        if req.crop is not None:
            rc, cur = orc.crop(cur, req.crop, req.gravity)
        if rc == 0 and req.resize is not None:
            rc, cur = orc.resize(cur, req.resize, 2000, 2000, req.simple)
        if rc == 0 and cur.shape[2] == 1:
            cur = orc.gray2bgr(cur)
        for flt in req.filters:
            if rc == 0:
                rc, cur = orc.filter(cur, flt, 0)
        if rc == 0 and placement:
            gx, gy, ox, oy, op = placement.split(",")
            rc, cur = orc.watermark(cur, overlay_frame(), gx, gy, int(ox), int(oy), int(op))
        if rc == 0 and req.need_flatten and cur.shape[2] == 4:
            cur = orc.blend_with_paper(cur)
        assert rc == 0, (query, rc)
        rc, ans = orc.jpeg_encode(cur, quality)
        assert rc == 0
        answers.append(ans)
    write_pool(path, answers)


def run_point(pool, mode, nproc, seconds, answers=None, broker_name=None, timeout=300, query=None, overlay=None, placement=None):
    d = tempfile.mkdtemp(prefix="impw_")
    how = "direct" if mode == "direct" else "broker:%s" % broker_name
    if query is not None:           # any request: tools/request_worker.c (broker only)
        cmd = lambda i: [REQUEST_WORKER, pool, str(seconds), str(i), d, how, query, overlay or "-", placement or "-"] + ([answers] if answers else [])
    else:
        cmd = lambda i: [HARNESS, pool, str(seconds), str(i), d, how] + ([answers] if answers else [])
    procs = [subprocess.Popen(cmd(i), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for i in range(nproc)]
    t_end = time.time() + timeout
    try:
        while sum(os.path.exists(os.path.join(d, "ready.%d" % i)) for i in range(nproc)) < nproc:
            dead = [p for p in procs if p.poll() is not None]
            if dead or time.time() > t_end:
                raise SystemExit("worker did not get ready: %r" % [p.stderr.read()[-400:] for p in dead])
            time.sleep(0.01)
        open(os.path.join(d, "go"), "w").close()
        out = []
        for p in procs:
            so, se = p.communicate(timeout=timeout)
            if p.returncode != 0:
                raise SystemExit("worker failed (%d): %s" % (p.returncode, se[-800:]))
            out.append(json.loads(so.strip().splitlines()[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        shutil.rmtree(d, ignore_errors=True)
    total = sum(r["requests"] for r in out)
    span = max(r["seconds"] for r in out)
    lat = sorted(out, key=lambda r: r["p50_us"])
    return {
        "mode": mode, "processes": nproc, "requests": total, "seconds": round(span, 3), "requests_per_s": round(total / span, 1),
        "p50_us": round(sum(r["p50_us"] * r["requests"] for r in out) / max(total, 1), 1),
        "p95_us": round(max(r["p95_us"] for r in out), 1), "p99_us": round(max(r["p99_us"] for r in out), 1),
        "mean_batch": round(sum(r["mean_batch"] * r["requests"] for r in out) / max(total, 1), 2),
        "mismatches": sum(r["mismatches"] for r in out), "checked": all(r["checked"] for r in out),
        "chain_timeouts": sum(r["chain_timeouts"] for r in out), "refused": sum(r["refused"] for r in out),
        "slowest_worker_p50_us": lat[-1]["p50_us"], "fastest_worker_p50_us": lat[0]["p50_us"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["direct", "broker"])
    ap.add_argument("procs", type=int, nargs="+")
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--gather-us", type=int, default=0)
    ap.add_argument("--pool", default=os.path.join(ROOT, "gpurun_out", "jpeg_pool.bin"))
    ap.add_argument("--answers", default=None)
    ap.add_argument("--hw-queues", type=int, default=0, help="GPU_MAX_HW_QUEUES for the broker (0: the runtime's default, 4)")
    ap.add_argument("--query", default=None, help="the request's query string (default resize=224,0 through worker_harness)")
    ap.add_argument("--watermark", default=None, metavar="GX,GY,OX,OY,OPACITY", help="a location watermark with this placement")
    ap.add_argument("--check", action="store_true", help="with --query: compare every answer with the oracle's file")
    args = ap.parse_args()
    if args.pool == "png":               # the same 64 files as PNG uploads (broker only, through --query's worker)
        if args.mode != "broker":
            ap.error("--pool png: broker mode only (the direct worker decodes JPEG)")
        args.pool = os.path.join(os.path.dirname(ap.get_default("pool")), "png_pool.bin")   # (beside the JPEG pool)
        args.query = args.query if args.query is not None else "resize=224,0"
        os.makedirs(os.path.dirname(args.pool), exist_ok=True)
        make_png_pool(args.pool)
    else:
        os.makedirs(os.path.dirname(args.pool), exist_ok=True)
        make_pool(args.pool)
    overlay = None
    if args.query is not None or args.watermark:
        if args.mode != "broker":
            ap.error("--query / --watermark: broker mode only")
        args.query = args.query if args.query is not None else "resize=224,0"
        build_request_worker()
        tmp = tempfile.mkdtemp(prefix="impq_")
        if args.watermark:
            overlay = os.path.join(tmp, "overlay.bin")
            write_overlay(overlay)
        if args.check:
            args.answers = os.path.join(tmp, "answers.bin")
            oracle_answers(args.pool, args.query, args.watermark, args.answers)
    for n in args.procs:
        if args.mode == "direct" and n > 6:
            print(json.dumps({"mode": "direct", "processes": n, "skipped": "more than 6 processes on the card"}), flush=True)
            continue
        broker = None
        name = "/impgpu-scaling-%d" % os.getpid()
        if args.mode == "broker":
            env = {}
            if args.hw_queues:
                env["GPU_MAX_HW_QUEUES"] = str(args.hw_queues)
            broker = start_broker(name, args.threads, args.gather_us, env=env or None)
        try:
            r = run_point(args.pool, args.mode, n, args.seconds, args.answers, name, query=args.query, overlay=overlay,
                          placement=args.watermark)
            if args.query is not None:
                r["query"] = args.query
                r["watermark"] = args.watermark
            if broker:
                r["broker_threads"] = args.threads
                r["gather_us"] = args.gather_us
                r["hw_queues"] = args.hw_queues or 8
            print(json.dumps(r), flush=True)
        finally:
            if broker:
                err = stop_broker(broker)
                for ln in err.strip().splitlines()[-2:]:
                    print("# " + ln, flush=True)


if __name__ == "__main__":
    main()
