"""Python mirror of the reference's operator interface (bridge.h / filters.h) over libimpgpu.so.

`Image` stands for the IplImage* the reference hands from operator to operator; its methods
carry the reference's names and take the reference's argument strings.  Methods return the
IMP_* code (0 = IMP_OK) exactly like the C functions, so tests read like calls into bridge.c.
numpy arrays are H x W x C uint8 in B,G,R[,A] order.
"""
import ctypes as C

import numpy as np

from ._lib import lib, CConfig, CJob, ImpError

IMP_OK = 0
IMP_ERROR_UNSUPPORTED = 1
IMP_ERROR_MALLOC_FAILED = 2
IMP_ERROR_DECODE_FAILED = 3
IMP_ERROR_INVALID_ARGS = 50
IMP_ERROR_UPSCALE = 51
IMP_ERROR_NO_SUCH_FILTER = 52
IMP_ERROR_NO_SUCH_WATERMARK = 53
IMP_ERROR_TOO_BIG_TARGET = 54
IMP_ERROR_TOO_MUCH_FILTERS = 55
IMP_ERROR_DEVICE = 90
INTER_NN, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4

# impgpu_*_jpeg_ex accept mask (include/impgpu.h)
JPEG_PROGRESSIVE = 1
# impgpu_*_png_ex accept masks (include/impgpu.h)
PNG_PALETTE = 1
PNG_LOW_GRAY = 2
PNG_ADAM7 = 4
PNG_ALL = PNG_PALETTE | PNG_LOW_GRAY | PNG_ADAM7
PNG_DEVICE_INFLATE = 8          # not part of PNG_ALL: how files are decoded (k_png_inflate), not which are taken
# impgpu_*_decode_gif_ex flags (include/impgpu.h)
GIF_SPLIT = 1                   # cut every page at its clear codes, a wavefront per segment (k_gif_lzw_scan / _len / _emit)
GIF_SPLIT_MIN_BYTES = 2048      # IMPGPU_GIF_SPLIT_MIN_BYTES: a clear code nearer than this to its segment's start is no cut
GIF_ENC_QUANTIZE = 1            # IMPGPU_GIF_ENC_QUANTIZE: a frame past 256 colours gets a median-cut table (the _ex encode calls)
GIF_ENC_DELTA = 2               # IMPGPU_GIF_ENC_DELTA: pixels equal to the previous frame's are written transparent, frames shrink to what changed (the _ex2 calls)
GIF_ENC_SEGMENT = 8192          # IMPGPU_GIF_ENC_SEGMENT: the pixels between two clear codes of an encoded page (segment = 0)


def _b(s):
    return None if s is None else (s if isinstance(s, bytes) else str(s).encode())


def env_start(device=-1):
    """OnEnvStart (bridge.c:10). Raises when no GPU is usable."""
    rc = lib.impgpu_env_start(device)
    if rc:
        raise ImpError(rc, "impgpu_env_start")
    return lib.impgpu_env_device()


def env_destroy():
    lib.impgpu_env_destroy()


def sync():
    rc = lib.impgpu_sync()
    if rc:
        raise ImpError(rc, "impgpu_sync")


class Config:
    """The Config fields the operators read (required.h:108-118); defaults of module.c:168-187."""

    def __init__(self, max_w=2000, max_h=2000, max_filters=5, allow_experiments=False):
        self.c = CConfig()
        self.c.max_target_w = max_w
        self.c.max_target_h = max_h
        self.c.max_filters_count = max_filters
        self.c.allow_experiments = int(bool(allow_experiments))
        self.c.watermark_opacity = 100
        self.c.watermark_gravity_x = b"l"
        self.c.watermark_gravity_y = b"t"
        self.c.watermark_offset_x = 0
        self.c.watermark_offset_y = 0
        self.c.watermark = None

    def prepare_watermark(self, overlay, gravity_x="r", gravity_y="b", offset_x=0, offset_y=0, opacity=100):
        """PrepareWatermark (bridge.c:199-237) minus file read / decode: upload the decoded overlay once."""
        ov = np.ascontiguousarray(overlay, dtype=np.uint8)
        if ov.ndim == 2:
            ov = ov[:, :, None]
        h, w, c = ov.shape
        rc = lib.impgpu_prepare_watermark(C.byref(self.c), ov.ctypes.data, w, h, c, w * c)
        if rc:
            return rc
        self.c.watermark_gravity_x = _b(gravity_x)
        self.c.watermark_gravity_y = _b(gravity_y)
        self.c.watermark_offset_x = offset_x
        self.c.watermark_offset_y = offset_y
        self.c.watermark_opacity = opacity
        return IMP_OK

    def release(self):
        if self.c.watermark:
            h = C.c_void_p(self.c.watermark)
            lib.impgpu_image_release(C.byref(h))
            self.c.watermark = None


class Image:
    """Device-resident frame (impgpu_image*)."""

    def __init__(self, arr=None, handle=None):
        self.h = C.c_void_p()
        if handle is not None:
            self.h = C.c_void_p(handle)
            return
        a = np.ascontiguousarray(arr, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        hh, ww, cc = a.shape
        rc = lib.impgpu_image_upload(a.ctypes.data, ww, hh, cc, ww * cc, C.byref(self.h))
        if rc:
            raise ImpError(rc, "impgpu_image_upload")

    @classmethod
    def wrap(cls, device_ptr, width, height, channels, step):
        h = C.c_void_p()
        rc = lib.impgpu_image_wrap(C.c_void_p(device_ptr), width, height, channels, step, C.byref(h))
        if rc:
            raise ImpError(rc, "impgpu_image_wrap")
        return cls(handle=h.value)

    @classmethod
    def decode_jpeg(cls, blob):
        """cvDecodeImage(&rawencoded, -1) for a JPEG blob (bridge.c:545-552), on the device -> (code, Image or None)."""
        h = C.c_void_p()
        rc = lib.impgpu_image_decode_jpeg(bytes(blob), len(blob), C.byref(h))
        return rc, (cls(handle=h.value) if rc == 0 else None)

    @classmethod
    def decode_jpeg_ex(cls, blob, accept):
        """impgpu_image_decode_jpeg_ex: decode_jpeg that also takes the kinds of `accept` (JPEG_PROGRESSIVE) -> (code, Image or None)."""
        h = C.c_void_p()
        rc = lib.impgpu_image_decode_jpeg_ex(bytes(blob), len(blob), int(accept), C.byref(h))
        return rc, (cls(handle=h.value) if rc == 0 else None)

    @classmethod
    def decode_png(cls, blob):
        """cvDecodeImage(&rawencoded, -1) for a PNG blob (bridge.c:545-552): host inflate, filters undone on the device
        -> (code, Image or None)."""
        h = C.c_void_p()
        rc = lib.impgpu_image_decode_png(bytes(blob), len(blob), C.byref(h))
        return rc, (cls(handle=h.value) if rc == 0 else None)

    @classmethod
    def decode_png_ex(cls, blob, accept):
        """impgpu_image_decode_png_ex: decode_png that also takes the kinds of `accept` (PNG_PALETTE | PNG_LOW_GRAY | PNG_ADAM7)
        -> (code, Image or None)."""
        h = C.c_void_p()
        rc = lib.impgpu_image_decode_png_ex(bytes(blob), len(blob), int(accept), C.byref(h))
        return rc, (cls(handle=h.value) if rc == 0 else None)

    @classmethod
    def album(cls, frames):
        """The frames of one animation (same geometry) as ONE handle: every operator then runs once for all of them
        (impgpu_album_upload; Album, required.h:56-66)."""
        arrs = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        arrs = [a[:, :, None] if a.ndim == 2 else a for a in arrs]
        hh, ww, cc = arrs[0].shape
        if any(a.shape != (hh, ww, cc) for a in arrs):
            raise ValueError("album frames differ in geometry")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        h = C.c_void_p()
        rc = lib.impgpu_album_upload(ptrs, len(arrs), ww, hh, cc, None, C.byref(h))
        if rc:
            raise ImpError(rc, "impgpu_album_upload")
        return cls(handle=h.value)

    @property
    def count(self):
        return lib.impgpu_album_count(self.h)

    def frames(self):
        """Every frame of the album -> list of HxWxC arrays (impgpu_album_download: one copy, one wait)."""
        hh, ww, cc = self.shape
        outs = [np.empty((hh, ww, cc), dtype=np.uint8) for _ in range(self.count)]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        rc = lib.impgpu_album_download(self.h, ptrs, None)
        if rc:
            raise ImpError(rc, "impgpu_album_download")
        return outs

    def frames_fi(self, bpp, pitch=None, fill=0):
        """Every frame in FreeImage layout (impgpu_album_download_fi: bottom-up, `pitch` bytes per row -- FreeImage's own
        rule when None) -> (code, list of h x pitch arrays that held `fill` before)."""
        hh, ww, cc = self.shape
        pitch = (ww * bpp // 8 + 3) & ~3 if pitch is None else pitch
        outs = [np.full((hh, pitch), fill, dtype=np.uint8) for _ in range(self.count)]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        rc = lib.impgpu_album_download_fi(self.h, int(bpp), ptrs, (C.c_int * len(outs))(*[pitch] * len(outs)))
        return rc, outs

    def encode_jpeg(self, quality=95):
        """cvEncodeImage(".jpg", frame, {CV_IMWRITE_JPEG_QUALITY, quality}) (bridge.c:704) on the device -> (code, file bytes or None)."""
        hh, ww, cc = self.shape
        cap = lib.impgpu_jpeg_encode_bound(ww, hh, cc)
        buf = np.empty(max(1, cap), dtype=np.uint8)
        n = C.c_size_t()
        rc = lib.impgpu_image_encode_jpeg(self.h, int(quality), buf.ctypes.data, cap, C.byref(n))
        return rc, (buf[: n.value].tobytes() if rc == 0 else None)

    def encode_png(self, level=9):
        """cvEncodeImage(".png", frame, {CV_IMWRITE_PNG_COMPRESSION, level}) (bridge.c:704) on the device -> (code, file bytes or None)."""
        hh, ww, cc = self.shape
        cap = lib.impgpu_png_encode_bound(ww, hh, cc)
        buf = np.empty(max(1, cap), dtype=np.uint8)
        n = C.c_size_t()
        rc = lib.impgpu_image_encode_png(self.h, int(level), buf.ctypes.data, cap, C.byref(n))
        return rc, (buf[: n.value].tobytes() if rc == 0 else None)

    def release(self):
        if self.h:
            lib.impgpu_image_release(C.byref(self.h))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    @property
    def shape(self):
        return (lib.impgpu_image_height(self.h), lib.impgpu_image_width(self.h), lib.impgpu_image_channels(self.h))

    @property
    def device_ptr(self):
        return lib.impgpu_image_device_ptr(self.h)

    @property
    def step(self):
        """Device row pitch in bytes (cvCreateImage's 4-byte alignment rule)."""
        return lib.impgpu_image_step(self.h)

    def numpy(self):
        hh, ww, cc = self.shape
        out = np.empty((hh, ww, cc), dtype=np.uint8)
        rc = lib.impgpu_image_download(self.h, out.ctypes.data, ww * cc)
        if rc:
            raise ImpError(rc, "impgpu_image_download")
        return out

    def clone(self):
        h = C.c_void_p()
        rc = lib.impgpu_image_clone(self.h, C.byref(h))
        if rc:
            raise ImpError(rc, "impgpu_image_clone")
        return Image(handle=h.value)

    # ---- the reference's operators ----
    def crop(self, args, gravity=None):
        """Crop(IplImage**, args, gravity), bridge.c:18."""
        return lib.impgpu_crop(C.byref(self.h), _b(args), _b(gravity))

    def resize(self, args, config=None, simple=0):
        """Resize(IplImage**, args, config, simple), bridge.c:143."""
        cfg = config or Config()
        return lib.impgpu_resize(C.byref(self.h), _b(args), C.byref(cfg.c), simple)

    def cv_resize(self, width, height, interpolation):
        """cvResize(image, resized, filter), bridge.c:191."""
        return lib.impgpu_cv_resize(C.byref(self.h), width, height, interpolation)

    def filter(self, request, allow_experiments=1):
        """Filter(IplImage**, "name=args", allowExperiments), filters.c:43."""
        return lib.impgpu_filter(C.byref(self.h), _b(request), int(allow_experiments))

    def watermark(self, config):
        """Watermark(IplImage*, Config*), bridge.c:239."""
        return lib.impgpu_watermark(self.h, C.byref(config.c))

    def blend_with_paper(self):
        """BlendWithPaper(IplImage*), filters.c:666."""
        return lib.impgpu_blend_with_paper(self.h)

    def calc_perceived_brightness(self):
        """CalcPerceivedBrightness(IplImage*), filters.c:707."""
        out = C.c_float()
        rc = lib.impgpu_calc_perceived_brightness(self.h, C.byref(out))
        if rc:
            raise ImpError(rc, "impgpu_calc_perceived_brightness")
        return out.value

    def ascii(self, args=""):
        """ASCII(IplImage*, args, pool), filters.c:488."""
        hh, ww, _ = self.shape
        cap = (ww + 1) * hh
        buf = (C.c_ubyte * cap)()
        n = C.c_long()
        rc = lib.impgpu_ascii(self.h, _b(args), buf, cap, C.byref(n))
        if rc:
            raise ImpError(rc, "impgpu_ascii")
        return bytes(buf[: n.value])

    def gray2bgr(self):
        return lib.impgpu_gray2bgr(C.byref(self.h))

    def rgb2hsv(self):
        return lib.impgpu_rgb2hsv(self.h)

    def hsv2rgb(self):
        return lib.impgpu_hsv2rgb(self.h)


def _job(job, crop=None, gravity=None, resize=None, simple=0, filters=(), need_flatten=0):
    """Fill a CJob; returns the filter array, which must outlive the call."""
    job.crop = _b(crop)
    job.gravity = _b(gravity)
    job.resize = _b(resize)
    job.simple = simple
    arr = (C.c_char_p * max(1, len(filters)))(*[_b(f) for f in filters])
    job.filters = arr
    job.filter_count = len(filters)
    job.need_flatten = need_flatten
    return arr


def run_ops(image, config, crop=None, gravity=None, resize=None, simple=0, filters=(), need_flatten=0):
    """RunJob's operator segment, bridge.c:574-656. Returns (code, step)."""
    job = CJob()
    keep = _job(job, crop, gravity, resize, simple, filters, need_flatten)  # noqa: F841
    step = C.c_int()
    rc = lib.impgpu_run_ops(C.byref(image.h), C.byref(job), C.byref(config.c), C.byref(step))
    return rc, step.value


def batch_run_ops(images, configs, jobs):
    """impgpu_batch_run_ops: run_ops for request i = (images[i], configs[i], **jobs[i]) at once.  The Image objects take
    their new handles like run_ops' do.  Returns ([(code, step)], launches)."""
    n = len(images)
    if len(configs) != n or len(jobs) != n:
        raise ValueError("images, configs and jobs differ in length")
    handles = (C.c_void_p * max(1, n))(*[im.h.value for im in images])
    cjobs = (CJob * max(1, n))()
    keep = [_job(cjobs[i], **jobs[i]) for i in range(n)]  # noqa: F841
    cfgs = (C.POINTER(CConfig) * max(1, n))(*[C.pointer(c.c) for c in configs])
    codes = (C.c_int * max(1, n))()
    steps = (C.c_int * max(1, n))()
    launches = C.c_int()
    rc = lib.impgpu_batch_run_ops(handles, cjobs, cfgs, n, codes, steps, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_run_ops")
    for i, im in enumerate(images):
        im.h = C.c_void_p(handles[i])
    return [(codes[i], steps[i]) for i in range(n)], launches.value


def _handle(im):
    """The handle of an Image, a bare handle (c_void_p / int) or None (a NULL entry)."""
    if im is None:
        return None
    h = getattr(im, "h", im)
    return getattr(h, "value", h)


def batch_calc_perceived_brightness(images):
    """impgpu_batch_calc_perceived_brightness: Image.calc_perceived_brightness of every frame in one call.  An entry may be
    None (a NULL handle: its code says so).  Returns (values, codes, launches); values[i] is None where codes[i] != 0."""
    n = len(images)
    handles = (C.c_void_p * max(1, n))(*[_handle(im) for im in images])
    vals = (C.c_float * max(1, n))()
    codes = (C.c_int * max(1, n))()
    launches = C.c_int()
    rc = lib.impgpu_batch_calc_perceived_brightness(handles, n, vals, codes, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_calc_perceived_brightness")
    return [vals[i] if codes[i] == 0 else None for i in range(n)], [codes[i] for i in range(n)], launches.value


def batch_ascii(images, args=None, capacities=None):
    """impgpu_batch_ascii: Image.ascii(args[i]) of every frame in one call; the frames are left in HSV.  `args` may be None
    (all ""), and so may any args[i]; an entry of `images` may be None.  `capacities` (tests) overrides the buffer sizes the
    call is told.  Returns (texts, codes, launches); texts[i] is None where codes[i] != 0."""
    n = len(images)
    if args is not None and len(args) != n:
        raise ValueError("images and args differ in length")
    handles = (C.c_void_p * max(1, n))(*[_handle(im) for im in images])
    cargs = None if args is None else (C.c_char_p * max(1, n))(*[_b(a) for a in args])
    need = []
    for im in images:
        hh, ww = (im.shape[0], im.shape[1]) if im is not None and hasattr(im, "shape") else (0, 0)
        need.append(max(1, (ww + 1) * hh))
    bufs = [(C.c_ubyte * k)() for k in need]
    outs = (C.c_void_p * max(1, n))(*[C.addressof(b) for b in bufs])
    caps = (C.c_long * max(1, n))(*(need if capacities is None else capacities))
    lens = (C.c_long * max(1, n))()
    codes = (C.c_int * max(1, n))()
    launches = C.c_int()
    rc = lib.impgpu_batch_ascii(handles, cargs, n, outs, caps, lens, codes, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_ascii")
    texts = [bytes(bufs[i][: lens[i]]) if codes[i] == 0 else None for i in range(n)]
    return texts, [codes[i] for i in range(n)], launches.value


def _frame_count(im):
    return 0 if _handle(im) is None else lib.impgpu_album_count(C.c_void_p(_handle(im)))


def batch_download_fi(images, bpps, pitches=None, fill=0):
    """impgpu_batch_download_fi: Image.frames_fi(bpps[i], pitches[i]) of every handle (albums and single images) in one call
    behind one wait.  An entry of `images` may be None; pitches[i] (None: FreeImage's own rule) is the row pitch of every
    bitmap of handle i.  Returns (bitmaps, codes, launches): bitmaps[i] is the list of handle i's h x pitch arrays, which
    held `fill` before."""
    n = len(images)
    if len(bpps) != n or (pitches is not None and len(pitches) != n):
        raise ValueError("images, bpps and pitches differ in length")
    outs, ptrs, rows = [], [], []
    for i, im in enumerate(images):
        hh, ww = (im.shape[0], im.shape[1]) if _handle(im) is not None else (0, 0)
        pitch = pitches[i] if pitches is not None and pitches[i] is not None else (ww * (int(bpps[i]) // 8) + 3) & ~3
        mine = [np.full((hh, max(0, pitch)), fill, dtype=np.uint8) for _ in range(_frame_count(im))]
        outs.append(mine)
        ptrs += [o.ctypes.data for o in mine]
        rows += [pitch] * len(mine)
    m = len(ptrs)
    handles = (C.c_void_p * max(1, n))(*[_handle(im) for im in images])
    codes = (C.c_int * max(1, n))()
    launches = C.c_int()
    rc = lib.impgpu_batch_download_fi(handles, (C.c_int * max(1, n))(*[int(b) for b in bpps]), n, (C.c_void_p * max(1, m))(*ptrs),
                                      (C.c_int * max(1, m))(*rows), codes, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_download_fi")
    return outs, [codes[i] for i in range(n)], launches.value


def batch_album_download(images):
    """impgpu_batch_album_download: Image.frames() of every handle in one call behind one wait.  An entry may be None.
    Returns (frames, codes): frames[i] is the list of handle i's HxWxC arrays."""
    n = len(images)
    outs, ptrs, rows = [], [], []
    for im in images:
        hh, ww, cc = im.shape if _handle(im) is not None else (0, 0, 0)
        mine = [np.empty((hh, ww, cc), dtype=np.uint8) for _ in range(_frame_count(im))]
        outs.append(mine)
        ptrs += [o.ctypes.data for o in mine]
        rows += [ww * cc] * len(mine)
    m = len(ptrs)
    handles = (C.c_void_p * max(1, n))(*[_handle(im) for im in images])
    codes = (C.c_int * max(1, n))()
    rc = lib.impgpu_batch_album_download(handles, n, (C.c_void_p * max(1, m))(*ptrs), (C.c_int * max(1, m))(*rows), codes)
    if rc:
        raise ImpError(rc, "impgpu_batch_album_download")
    return outs, [codes[i] for i in range(n)]


def batch_decode_jpeg(blobs):
    """impgpu_batch_decode_jpeg -> [(code, Image or None)] in the order of `blobs`."""
    n = len(blobs)
    keep = [bytes(b) for b in blobs]
    arr = (C.c_char_p * n)(*keep)
    sizes = (C.c_size_t * n)(*[len(b) for b in keep])
    imgs = (C.c_void_p * n)()
    codes = (C.c_int * n)()
    rc = lib.impgpu_batch_decode_jpeg(arr, sizes, n, imgs, codes)
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_jpeg")
    return [(codes[i], Image(handle=imgs[i]) if codes[i] == 0 else None) for i in range(n)]


def batch_decode_jpeg_ex(blobs, accept):
    """impgpu_batch_decode_jpeg_ex -> [(code, Image or None)] in the order of `blobs`."""
    n = len(blobs)
    keep = [bytes(b) for b in blobs]
    arr = (C.c_char_p * max(1, n))(*keep)
    sizes = (C.c_size_t * max(1, n))(*[len(b) for b in keep])
    imgs = (C.c_void_p * max(1, n))()
    codes = (C.c_int * max(1, n))()
    rc = lib.impgpu_batch_decode_jpeg_ex(arr, sizes, n, int(accept), imgs, codes)
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_jpeg_ex")
    return [(codes[i], Image(handle=imgs[i]) if codes[i] == 0 else None) for i in range(n)]


def batch_decode_jpeg_begin_finish_ex(blobs, accept, prepared=False, pending=False):
    """impgpu_batch_decode_jpeg_begin_ex (or, prepared=True, _prepared_begin_ex with every file whole) and _finish, one
    group -> ([(code, Image or None)], level launches of the group).  pending=True (prepared only): the frames are taken
    through impgpu_batch_decode_jpeg_pending ahead of the verdicts."""
    from ._lib import CJpegPrepared

    n = len(blobs)
    keep = [np.frombuffer(bytes(b), np.uint8) for b in blobs]
    h = C.c_void_p()
    if prepared:
        arr = (CJpegPrepared * n)()
        for i, b in enumerate(keep):
            arr[i].head, arr[i].head_size, arr[i].scan, arr[i].scan_size, arr[i].registered = b.ctypes.data, b.size, None, 0, 0
        rc = lib.impgpu_batch_decode_jpeg_prepared_begin_ex(arr, n, int(accept), C.byref(h))
    else:
        raw = [bytes(b) for b in blobs]
        arr = (C.c_char_p * n)(*raw)
        sizes = (C.c_size_t * n)(*[len(b) for b in raw])
        rc = lib.impgpu_batch_decode_jpeg_begin_ex(arr, sizes, n, int(accept), C.byref(h))
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_jpeg_begin_ex")
    early = (C.c_void_p * n)()
    if pending:
        rc = lib.impgpu_batch_decode_jpeg_pending(h, early)
        if rc:
            raise ImpError(rc, "impgpu_batch_decode_jpeg_pending")
    was = lib.impgpu_jpeg_profile(1)
    imgs = (C.c_void_p * n)()
    codes = (C.c_int * n)()
    rc = lib.impgpu_batch_decode_jpeg_finish(C.byref(h), imgs, codes)
    t = (C.c_double * 16)()
    lib.impgpu_jpeg_stage_times(t, 16)
    lib.impgpu_jpeg_profile(was)
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_jpeg_finish")
    out = []
    for i in range(n):
        handle = imgs[i] or early[i]
        im = Image(handle=handle) if handle else None
        if codes[i] != 0 and im is not None:
            im.release()
            im = None
        out.append((codes[i], im))
    return out, int(t[14])


def jpeg_info_ex(blob, accept):
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_jpeg_info_ex(bytes(blob), len(blob), int(accept), w, h, c)
    return rc, ((w.value, h.value, c.value) if rc == 0 else None)


def jpeg_counters():
    """impgpu_jpeg_counters -> a list of 16 counts"""
    c = (C.c_ulonglong * 16)()
    lib.impgpu_jpeg_counters(c, 16)
    return list(c)


def batch_decode_png(blobs):
    """impgpu_batch_decode_png -> ([(code, Image or None)] in the order of `blobs`, kernel launches of the call)."""
    n = len(blobs)
    keep = [bytes(b) for b in blobs]
    arr = (C.c_char_p * max(1, n))(*keep)
    sizes = (C.c_size_t * max(1, n))(*[len(b) for b in keep])
    imgs = (C.c_void_p * max(1, n))()
    codes = (C.c_int * max(1, n))()
    launches = C.c_int()
    rc = lib.impgpu_batch_decode_png(arr, sizes, n, imgs, codes, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_png")
    return [(codes[i], Image(handle=imgs[i]) if codes[i] == 0 else None) for i in range(n)], launches.value


def batch_decode_png_ex(blobs, accept):
    """impgpu_batch_decode_png_ex -> ([(code, Image or None)] in the order of `blobs`, kernel launches of the call)."""
    n = len(blobs)
    keep = [bytes(b) for b in blobs]
    arr = (C.c_char_p * max(1, n))(*keep)
    sizes = (C.c_size_t * max(1, n))(*[len(b) for b in keep])
    imgs = (C.c_void_p * max(1, n))()
    codes = (C.c_int * max(1, n))()
    launches = C.c_int()
    rc = lib.impgpu_batch_decode_png_ex(arr, sizes, n, int(accept), imgs, codes, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_png_ex")
    return [(codes[i], Image(handle=imgs[i]) if codes[i] == 0 else None) for i in range(n)], launches.value


def jpeg_unstuff(blob):
    """impgpu_jpeg_unstuff of libimpgpu_client.so (what a worker does on the way into its slot) -> (head, scan) or None when
    the file is to go as it is."""
    from .broker import clib

    blob = bytes(blob)
    out = np.empty(len(blob) + 2048, np.uint8)
    head, at, n, total = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    if not clib.impgpu_jpeg_unstuff(blob, len(blob), out.ctypes.data, out.size, C.byref(head), C.byref(at), C.byref(n), C.byref(total)):
        return None
    return out[:head.value].tobytes(), out[at.value:at.value + n.value].tobytes()


def batch_decode_jpeg_prepared(files, pinned=False):
    """impgpu_batch_decode_jpeg_prepared.  files: whole files (bytes) or (head, scan) pairs as jpeg_unstuff returns them;
    pinned: the scans are put into impgpu_host_alloc memory and handed over as `registered`."""
    from ._lib import CJpegPrepared

    n = len(files)
    arr = (CJpegPrepared * n)()
    keep, pins = [], []
    for i, f in enumerate(files):
        if isinstance(f, (bytes, bytearray)):
            b = np.frombuffer(bytes(f), np.uint8)
            keep.append(b)
            arr[i].head, arr[i].head_size, arr[i].scan, arr[i].scan_size, arr[i].registered = b.ctypes.data, b.size, None, 0, 0
            continue
        head, scan = f
        h = np.frombuffer(bytes(head), np.uint8)
        tail = 1024                                                # IMPGPU_JPEG_SCAN_TAIL
        if pinned:
            p = lib.impgpu_host_alloc(len(scan) + tail)
            if not p:
                raise ImpError(IMP_ERROR_DEVICE, "impgpu_host_alloc")
            pins.append(p)
            sc = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(len(scan) + tail,))
        else:
            sc = np.empty(len(scan) + tail, np.uint8)
        sc[:len(scan)] = np.frombuffer(bytes(scan), np.uint8)
        sc[len(scan):] = 0xFF
        keep += [h, sc]
        arr[i].head, arr[i].head_size, arr[i].scan, arr[i].scan_size, arr[i].registered = h.ctypes.data, h.size, sc.ctypes.data, len(scan), int(pinned)
    imgs = (C.c_void_p * n)()
    codes = (C.c_int * n)()
    try:
        rc = lib.impgpu_batch_decode_jpeg_prepared(arr, n, imgs, codes)
    finally:
        for p in pins:
            lib.impgpu_host_free(p)
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_jpeg_prepared")
    return [(codes[i], Image(handle=imgs[i]) if codes[i] == 0 else None) for i in range(n)]


def jpeg_request_one_wait(blob, config, quality=86, **ops):
    """A request end to end with ONE wait (round 5): the file's decode is begun on the thread's own stream, its frame taken
    ahead of the verdict (impgpu_batch_decode_jpeg_pending), the operators (**ops as for run_ops) and the answer's encode are
    enqueued behind it, and only then the verdict and the file are waited for.  Returns (code, file bytes or None): a code
    other than 0 is the decode's -- the caller falls back exactly as after impgpu_image_decode_jpeg."""
    from ._lib import CJpegPrepared

    keep = np.frombuffer(bytes(blob), np.uint8)
    f = (CJpegPrepared * 1)()
    f[0].head, f[0].head_size, f[0].scan, f[0].scan_size, f[0].registered = keep.ctypes.data, keep.size, None, 0, 0
    batch = C.c_void_p()
    rc = lib.impgpu_batch_decode_jpeg_prepared_begin(f, 1, C.byref(batch))
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_jpeg_prepared_begin")
    img = (C.c_void_p * 1)()
    code = (C.c_int * 1)()
    rc = lib.impgpu_batch_decode_jpeg_pending(batch, img)
    if rc or not img[0]:                                           # nothing to run ahead with: the two-wait form
        lib.impgpu_batch_decode_jpeg_finish(C.byref(batch), img, code)
        if code[0] or not img[0]:
            return code[0] or IMP_ERROR_DECODE_FAILED, None
        im = Image(handle=img[0])
        rc, _ = run_ops(im, config, **ops)
        out = im.encode_jpeg(quality) if rc == 0 else (rc, None)
        im.release()
        return out
    im = Image(handle=img[0])
    rc_ops, _ = run_ops(im, config, **ops)
    enc = C.c_void_p()
    rc_enc = IMP_ERROR_DEVICE
    if rc_ops == 0:
        hs = (C.c_void_p * 1)(im.h.value)
        rc_enc = lib.impgpu_batch_encode_jpeg_begin(hs, 1, int(quality), C.byref(enc))
    none = (C.c_void_p * 1)()
    rc = lib.impgpu_batch_decode_jpeg_finish(C.byref(batch), none, code)
    out = None
    ecode = (C.c_int * 1)()
    if rc_enc == 0:
        cap = lib.impgpu_jpeg_encode_bound(im.shape[1], im.shape[0], im.shape[2])
        buf = np.empty(cap, np.uint8)
        outs = (C.c_void_p * 1)(buf.ctypes.data)
        caps = (C.c_size_t * 1)(cap)
        lens = (C.c_size_t * 1)()
        rc2 = lib.impgpu_batch_encode_jpeg_finish(C.byref(enc), outs, caps, lens, ecode)
        if rc2 == 0 and ecode[0] == 0:
            out = buf[:lens[0]].tobytes()
    im.release()
    if rc or code[0]:
        return rc or code[0], None                                 # the frame did not hold the file's pixels: the answer is dropped
    if rc_ops:
        return rc_ops, None
    return (0, out) if out is not None else (rc_enc or ecode[0] or IMP_ERROR_DEVICE, None)


def _answer_arrays(images, bound, capacities=None, guard=0):
    """What a batch encode call takes for `images` (an entry may be None) -> (handles, capacities, buffers, their addresses,
    lengths, codes).  A capacity that `capacities` leaves open is bound(image); a buffer is `guard` bytes longer than its
    capacity and filled with 0xA5, so that _answer can tell what the call wrote; the codes start at -1."""
    m = max(1, len(images))
    caps = [(bound(a) if a is not None else 0) if capacities is None or capacities[i] is None else int(capacities[i]) for i, a in enumerate(images)]
    bufs = [np.full(max(1, c) + guard, 0xA5, np.uint8) for c in caps]
    return ((C.c_void_p * m)(*[_handle(a) for a in images]), (C.c_size_t * m)(*caps), bufs, (C.c_void_p * m)(*[b.ctypes.data for b in bufs]),
            (C.c_size_t * m)(), (C.c_int * m)(*([-1] * m)))


def batch_encode_jpeg(images, quality=95):
    """impgpu_batch_encode_jpeg -> [(code, file bytes or None)] in the order of `images`."""
    n = len(images)
    hs, ccaps, bufs, outs, lens, codes = _answer_arrays(images, lambda im: lib.impgpu_jpeg_encode_bound(im.shape[1], im.shape[0], im.shape[2]))
    rc = lib.impgpu_batch_encode_jpeg(hs, n, int(quality), outs, ccaps, lens, codes)
    if rc:
        raise ImpError(rc, "impgpu_batch_encode_jpeg")
    return [(codes[i], bufs[i][: lens[i]].tobytes() if codes[i] == 0 else None) for i in range(n)]


def batch_encode_png(images, level=9):
    """impgpu_batch_encode_png -> [(code, file bytes or None)] in the order of `images`."""
    n = len(images)
    hs, ccaps, bufs, outs, lens, codes = _answer_arrays(images, lambda im: lib.impgpu_png_encode_bound(im.shape[1], im.shape[0], im.shape[2]))
    rc = lib.impgpu_batch_encode_png(hs, n, int(level), outs, ccaps, lens, codes)
    if rc:
        raise ImpError(rc, "impgpu_batch_encode_png")
    return [(codes[i], bufs[i][: lens[i]].tobytes() if codes[i] == 0 else None) for i in range(n)]


def png_deflate(data):
    """impgpu_png_deflate (host, no device): the zlib stream libpng writes for these filtered scanlines -> (code, bytes)."""
    data = bytes(data)
    n = C.c_size_t()
    rc = lib.impgpu_png_deflate(data, len(data), None, 0, C.byref(n))
    if rc not in (0, IMP_ERROR_MALLOC_FAILED):
        return rc, None
    buf = np.empty(max(1, n.value), dtype=np.uint8)
    rc = lib.impgpu_png_deflate(data, len(data), buf.ctypes.data, n.value, C.byref(n))
    return rc, (buf[: n.value].tobytes() if rc == 0 else None)


def jpeg_info(blob):
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_jpeg_info(bytes(blob), len(blob), w, h, c)
    return rc, (w.value, h.value, c.value)


def png_info(blob):
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_png_info(bytes(blob), len(blob), w, h, c)
    return rc, (w.value, h.value, c.value)


def png_info_ex(blob, accept):
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_png_info_ex(bytes(blob), len(blob), int(accept), w, h, c)
    return rc, (w.value, h.value, c.value)


def png_scanlines_ex(blob, accept):
    """impgpu_png_scanlines_ex (host, no device): the filtered bytes of every non-empty pass -> (code, bytes or None)"""
    n = C.c_size_t(0)
    rc = lib.impgpu_png_scanlines_ex(bytes(blob), len(blob), int(accept), None, 0, C.byref(n))
    if rc != IMP_ERROR_MALLOC_FAILED:
        return rc, None
    buf = np.zeros(max(1, n.value), np.uint8)
    rc = lib.impgpu_png_scanlines_ex(bytes(blob), len(blob), int(accept), buf.ctypes.data, buf.size, C.byref(n))
    return rc, (buf[: n.value].tobytes() if rc == 0 else None)


def png_inflate_lanes(stream, out_size):
    """impgpu_png_inflate_lanes (host, no device): the device inflate's rounds, lane after lane, on one zlib stream into exactly
    out_size bytes -> (code, status word, bytes or None)"""
    stream = bytes(stream)
    buf = np.zeros(max(int(out_size), 1), np.uint8)
    st = C.c_int(-1)
    rc = lib.impgpu_png_inflate_lanes(stream, len(stream), buf.ctypes.data, int(out_size), C.byref(st))
    return rc, st.value, (buf[:int(out_size)].tobytes() if rc == 0 else None)


def png_stage_times():
    """the calling thread's last decode_png: host microseconds (header, chunks + CRC + inflate, check + enqueue), scanline bytes"""
    t = (C.c_double * 4)()
    lib.impgpu_png_stage_times(t, 4)
    return list(t)


def crop_geometry(width, height, args, gravity=None):
    x, y, w, h = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_crop_geometry(width, height, _b(args), _b(gravity), x, y, w, h)
    return rc, (x.value, y.value, w.value, h.value)


def resize_geometry(width, height, args, config=None, simple=0):
    cfg = config or Config()
    w, h, i = C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_resize_geometry(width, height, _b(args), C.byref(cfg.c), simple, w, h, i)
    return rc, (w.value, h.value, i.value)


def filter_check(request, allow_experiments=1):
    return lib.impgpu_filter_check(_b(request), int(allow_experiments))


def check_destructive(request):
    return lib.impgpu_check_destructive(_b(request))


def blur_form(width, height, channels, sigma):
    """impgpu_blur_form -> (form, planes): 0 a lone form, 1 k_blur_fused4, 2 / 3 the one- / two-pass matrix-unit form."""
    planes = C.c_int()
    return lib.impgpu_blur_form(width, height, channels, float(sigma), planes), planes.value


def batch_cv_resize(src_ptr, src_stride, sw, sh, sstep, dst_ptr, dst_stride, dw, dh, dstep, channels, count,
                    interpolation, stream=None):
    rc = lib.impgpu_batch_cv_resize(C.c_void_p(src_ptr), src_stride, sw, sh, sstep, C.c_void_p(dst_ptr), dst_stride,
                                    dw, dh, dstep, channels, count, interpolation, C.c_void_p(stream or 0))
    if rc:
        raise ImpError(rc, "impgpu_batch_cv_resize")


class ResizeItem(C.Structure):
    """impgpu_resize_item (include/impgpu.h)."""
    _fields_ = [("src", C.c_void_p), ("src_width", C.c_int), ("src_height", C.c_int), ("src_step", C.c_int),
                ("dst", C.c_void_p), ("dst_width", C.c_int), ("dst_height", C.c_int), ("dst_step", C.c_int)]


def batch_resize_mixed(items, channels, simple=False, stream=None, count_launches=False):
    """items: [(src_ptr, sw, sh, sstep, dst_ptr, dw, dh, dstep)] of frames resident in HBM; returns the IMP_* code, or
    (code, kernels enqueued) with count_launches=True."""
    arr = (ResizeItem * len(items))(*[ResizeItem(*it) for it in items])
    if not count_launches:
        return lib.impgpu_batch_resize_mixed(arr, len(items), channels, int(simple), C.c_void_p(stream or 0))
    launches = C.c_int(-1)
    rc = lib.impgpu_batch_resize_mixed_ex(arr, len(items), channels, int(simple), C.c_void_p(stream or 0), C.byref(launches))
    return rc, launches.value


def batch_resize_rotate_watermark(src_ptr, src_stride, sw, sh, sstep, dst_ptr, dst_stride, dstep, rw, rh, rotate,
                                  config, channels, count, stream=None):
    rc = lib.impgpu_batch_resize_rotate_watermark(C.c_void_p(src_ptr), src_stride, sw, sh, sstep, C.c_void_p(dst_ptr),
                                                  dst_stride, dstep, rw, rh, rotate, C.byref(config.c), channels,
                                                  count, C.c_void_p(stream or 0))
    if rc:
        raise ImpError(rc, "impgpu_batch_resize_rotate_watermark")


def gif_page_array(pages):
    """Page dicts (see gif_compose) -> (impgpu_gif_page array, the arrays it points into)."""
    from ._lib import CGifPage
    keep = []
    arr = (CGifPage * max(1, len(pages)))()
    for i, p in enumerate(pages):
        idx = np.ascontiguousarray(p["indices"], dtype=np.uint8)
        pal = np.ascontiguousarray(p["palette"], dtype=np.uint8)
        keep += [idx, pal]
        arr[i].indices = idx.ctypes.data
        arr[i].width = int(p["width"]); arr[i].height = idx.shape[0]; arr[i].pitch = idx.shape[1]
        arr[i].left = int(p.get("left", 0)); arr[i].top = int(p.get("top", 0))
        arr[i].dispose = int(p.get("dispose", 0)); arr[i].transparency_key = int(p.get("key", -1))
        arr[i].palette = pal.ctypes.data
    return arr, keep


def batch_gif_compose(sets, count=None):
    """impgpu_batch_gif_compose: sets = [(pages, destructive, page), ...] (pages as for gif_compose) -> (code, [album Image or
    None ...], [codes], launches).  `count` overrides the count passed to the library (its argument checks)."""
    from ._lib import CGifSet
    n = len(sets)
    arr = (CGifSet * max(1, n))()
    keep = []
    for i, (pages, destructive, page) in enumerate(sets):
        if pages is not None:
            pa, k = gif_page_array(pages)
            keep += [pa, k]
            arr[i].pages = pa
            arr[i].count = len(pages)
        arr[i].destructive, arr[i].page = int(bool(destructive)), int(page)
    m = max(1, n if count is None else count)
    outs = (C.c_void_p * m)()
    codes = (C.c_int * m)(*([-1] * m))
    launches = C.c_int(-1)
    rc = lib.impgpu_batch_gif_compose(arr, n if count is None else count, outs, codes, C.byref(launches))
    return rc, [Image(handle=outs[i]) if outs[i] else None for i in range(n)], list(codes[:n]), launches.value


def gif_compose(pages, destructive=False, page=-1, album=False):
    """LoadGIF's compositing loop (advancedio.c:204-247) on the device.  pages: dicts with `indices` (h x pitch uint8,
    FreeImage scanline order), `width`, `left`, `top`, `dispose`, `key`, `palette` (256 x 4 uint8, B,G,R,reserved).
    Returns (code, [Image ...]): every page, or just the requested one; album=True -> (code, one album Image)."""
    arr, keep = gif_page_array(pages)
    nout = 1 if page >= 0 else len(pages)
    outs = (C.c_void_p * max(1, nout))()
    if album:
        rc = lib.impgpu_gif_compose_album(arr, len(pages), int(bool(destructive)), int(page), outs)
        return rc, (Image(handle=outs[0]) if rc == 0 else None)
    rc = lib.impgpu_gif_compose(arr, len(pages), int(bool(destructive)), int(page), outs)
    if rc:
        return rc, []
    return 0, [Image(handle=outs[i]) for i in range(nout)]


def decode_gif(blob, destructive=False, page=-1, flags=0):
    """impgpu_image_decode_gif_ex: the GIF FILE -> (code, album Image or None): the container walk on the host, the LZW pages
    (k_gif_lzw; with flags = GIF_SPLIT cut at their clear codes, a wavefront per segment) and LoadGIF's compositing loop on
    the device."""
    blob = bytes(blob)
    out = C.c_void_p()
    rc = lib.impgpu_image_decode_gif_ex(blob, len(blob), int(bool(destructive)), int(page), int(flags), C.byref(out))
    return rc, (Image(handle=out.value) if rc == 0 and out.value else None)


def batch_decode_gif(files, count=None, flags=0):
    """impgpu_batch_decode_gif_ex: files = [(blob, destructive, page), ...] -> (code, [album Image or None ...], [codes],
    launches).  `count` overrides the count passed to the library (its argument checks); flags: 0 or GIF_SPLIT."""
    n = len(files)
    m = max(1, n if count is None else count)
    keep = [bytes(f[0]) for f in files]
    blobs = (C.c_char_p * m)(*keep)
    sizes = (C.c_size_t * m)(*[len(b) for b in keep])
    destr = (C.c_int * m)(*[int(bool(f[1])) for f in files])
    pages = (C.c_int * m)(*[int(f[2]) for f in files])
    outs = (C.c_void_p * m)()
    codes = (C.c_int * m)(*([-1] * m))
    launches = C.c_int(-1)
    rc = lib.impgpu_batch_decode_gif_ex(blobs, sizes, destr, pages, n if count is None else count, int(flags), outs, codes, C.byref(launches))
    return rc, [Image(handle=outs[i]) if outs[i] else None for i in range(n)], list(codes[:n]), launches.value


def gif_info(blob):
    """impgpu_gif_info (host, no device) -> (code, (pages, canvas width, canvas height))"""
    n, w, h = C.c_int(), C.c_int(), C.c_int()
    rc = lib.impgpu_gif_info(bytes(blob), len(blob), n, w, h)
    return rc, (n.value, w.value, h.value)


def gif_pages(blob, how=0):
    """impgpu_gif_pages (host, no device): every page's index plane (bottom-up, pitch (w + 3) & ~3), one after the other
    -> (code, bytes or None).  how = 0: a plain sequential LZW decoder; 1: the kernel's rounds run on the host."""
    blob = bytes(blob)
    n = C.c_size_t(0)
    rc = lib.impgpu_gif_pages(blob, len(blob), int(how), None, 0, C.byref(n))
    if rc != IMP_ERROR_MALLOC_FAILED:
        return rc, None
    buf = np.full(max(1, n.value), 0xA5, np.uint8)
    rc = lib.impgpu_gif_pages(blob, len(blob), int(how), buf.ctypes.data, n.value, C.byref(n))
    return rc, (buf[: n.value].tobytes() if rc == 0 else None)


def gif_pages_split(blob):
    """impgpu_gif_pages_split (host, no device): gif_pages' planes made by the GIF_SPLIT route's three passes, the kernels'
    own lane code run one lane after the other -> (code, bytes or None, [segments per page] or None when the container
    was not taken)."""
    blob = bytes(blob)
    n = C.c_size_t(0)
    rc = lib.impgpu_gif_pages_split(blob, len(blob), None, 0, C.byref(n), None, 0)
    if rc != IMP_ERROR_MALLOC_FAILED:
        return rc, None, None
    pages = gif_info(blob)[1][0]
    buf = np.full(max(1, n.value), 0xA5, np.uint8)
    segs = (C.c_int * max(1, pages))()
    rc = lib.impgpu_gif_pages_split(blob, len(blob), buf.ctypes.data, n.value, C.byref(n), segs, pages)
    return rc, (buf[: n.value].tobytes() if rc == 0 else None), list(segs[:pages])


IP_ = C.POINTER(C.c_int)


def _ints(values):
    return None if values is None else (C.c_int * max(1, len(values)))(*[int(v) for v in values])


def _answer(rc, buf, length):
    """(code, the file or None, *length, whether every byte the call had no business writing still holds the fill)"""
    n = length.value
    written = n if rc == 0 else 0
    return rc, (buf[:n].tobytes() if rc == 0 else None), n, bool((buf[written:] == 0xA5).all())


def gif_encode_bound(width, height, frames):
    """impgpu_gif_encode_bound: a size no GIF file of that album exceeds (0: a geometry the encoder refuses)"""
    return lib.impgpu_gif_encode_bound(int(width), int(height), int(frames))


def encode_gif(album, time_ms=None, dispose=None, loop_count=-1, segment=0, capacity=None, guard=64, flags=None, delta=False):
    """impgpu_album_encode_gif: the album (or single image) as a GIF file written on the device -- exact palette, LZW cut into
    segments of `segment` pixels, a wavefront each -> (code, bytes or None, length, intact).  `capacity` defaults to
    gif_encode_bound; `guard` bytes behind it are checked: intact = nothing at or behind out[length] (out[0] when the call
    failed) was written.  flags: None = the call itself; a number = impgpu_album_encode_gif_ex with those flags
    (GIF_ENC_QUANTIZE: frames past 256 colours are quantised on the device).  delta=True: impgpu_album_encode_gif_ex2 with
    those flags (0 for None) and GIF_ENC_DELTA."""
    cap = gif_encode_bound(album.shape[1], album.shape[0], album.count) if capacity is None else int(capacity)
    buf = np.full(cap + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    if delta:
        rc = lib.impgpu_album_encode_gif_ex2(album.h, _ints(time_ms), _ints(dispose), int(loop_count), int(segment), int(flags or 0) | GIF_ENC_DELTA,
                                             buf.ctypes.data, cap, C.byref(n))
    elif flags is None:
        rc = lib.impgpu_album_encode_gif(album.h, _ints(time_ms), _ints(dispose), int(loop_count), int(segment), buf.ctypes.data, cap, C.byref(n))
    else:
        rc = lib.impgpu_album_encode_gif_ex(album.h, _ints(time_ms), _ints(dispose), int(loop_count), int(segment), int(flags), buf.ctypes.data, cap,
                                            C.byref(n))
    return _answer(rc, buf, n)


def encode_gif_host(frames, time_ms=None, dispose=None, loop_count=-1, segment=0, capacity=None, guard=64, channels=None, flags=None, delta=False):
    """impgpu_gif_encode_host (no device): frames = HxWxC uint8 arrays of one geometry and one row pitch (views with padded
    rows are fine) -> (code, bytes or None, length, intact), as encode_gif.  flags: None, or impgpu_gif_encode_host_ex's;
    delta=True: impgpu_gif_encode_host_ex2 with those flags and GIF_ENC_DELTA."""
    first = frames[0]
    hh, ww, cc = first.shape
    step = first.strides[0]
    assert all(f.shape == first.shape and f.strides == (step, cc, 1) and f.dtype == np.uint8 for f in frames)
    ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    cap = gif_encode_bound(ww, hh, len(frames)) if capacity is None else int(capacity)
    buf = np.full(cap + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    if delta:
        rc = lib.impgpu_gif_encode_host_ex2(ptrs, len(frames), ww, hh, cc if channels is None else channels, step, _ints(time_ms), _ints(dispose),
                                            int(loop_count), int(segment), int(flags or 0) | GIF_ENC_DELTA, buf.ctypes.data, cap, C.byref(n))
    elif flags is None:
        rc = lib.impgpu_gif_encode_host(ptrs, len(frames), ww, hh, cc if channels is None else channels, step, _ints(time_ms), _ints(dispose),
                                        int(loop_count), int(segment), buf.ctypes.data, cap, C.byref(n))
    else:
        rc = lib.impgpu_gif_encode_host_ex(ptrs, len(frames), ww, hh, cc if channels is None else channels, step, _ints(time_ms), _ints(dispose),
                                           int(loop_count), int(segment), int(flags), buf.ctypes.data, cap, C.byref(n))
    return _answer(rc, buf, n)


def gif_quantize_host(frame):
    """impgpu_gif_quantize_host (no device): one HxWx3/4 uint8 frame (padded rows are fine) through the quantiser of
    GIF_ENC_QUANTIZE -> (code, (entries, 3) R,G,B table, transparent index or -1, HxW indices)"""
    hh, ww, cc = frame.shape
    assert frame.dtype == np.uint8 and frame.strides[1:] == (cc, 1)
    table = np.zeros((256, 3), np.uint8)
    indices = np.zeros((hh, ww), np.uint8)
    entries, tkey = C.c_int(0), C.c_int(0)
    rc = lib.impgpu_gif_quantize_host(frame.ctypes.data, ww, hh, cc, frame.strides[0], table.ctypes.data, C.byref(entries), C.byref(tkey),
                                      indices.ctypes.data)
    return rc, table[: entries.value].copy(), tkey.value, indices


def batch_encode_gif(albums, time_ms=None, dispose=None, loop_counts=None, segment=0, capacities=None, count=None, guard=64, flags=None, delta=False):
    """impgpu_batch_encode_gif: albums (Images; an entry may be None) -> (code, [(code, bytes or None, length, intact) ...],
    launches).  time_ms / dispose: per album a list or None; loop_counts default to -1; capacities to gif_encode_bound.
    flags: None, or impgpu_batch_encode_gif_ex's; delta=True: impgpu_batch_encode_gif_ex2 with those flags and GIF_ENC_DELTA."""
    n = len(albums)
    m = max(1, n)
    keep_t = [_ints(None if time_ms is None else time_ms[i]) for i in range(n)]
    keep_d = [_ints(None if dispose is None else dispose[i]) for i in range(n)]
    tarr = (IP_ * m)(*[C.cast(t, IP_) if t is not None else IP_() for t in keep_t])
    darr = (IP_ * m)(*[C.cast(d, IP_) if d is not None else IP_() for d in keep_d])
    loops = (C.c_int * m)(*[-1 if loop_counts is None else int(loop_counts[i]) for i in range(n)])
    handles, carr, bufs, outs, lens, codes = _answer_arrays(albums, lambda a: gif_encode_bound(a.shape[1], a.shape[0], a.count), capacities, guard)
    launches = C.c_int(-1)
    if delta:
        rc = lib.impgpu_batch_encode_gif_ex2(handles, tarr, darr, loops, n if count is None else count, int(segment), int(flags or 0) | GIF_ENC_DELTA, outs,
                                             carr, lens, codes, C.byref(launches))
    elif flags is None:
        rc = lib.impgpu_batch_encode_gif(handles, tarr, darr, loops, n if count is None else count, int(segment), outs, carr, lens, codes,
                                         C.byref(launches))
    else:                                                                # impgpu_batch_encode_gif_ex
        rc = lib.impgpu_batch_encode_gif_ex(handles, tarr, darr, loops, n if count is None else count, int(segment), int(flags), outs, carr, lens,
                                            codes, C.byref(launches))
    return rc, [_answer(codes[i], bufs[i], C.c_size_t(lens[i])) for i in range(n)], launches.value


WEBP_TILE_BITS = 4                            # IMPGPU_WEBP_TILE_BITS
WEBP_ENC_BACKREFS = 1                         # IMPGPU_WEBP_ENC_BACKREFS
WEBP_MIN_MATCH = 3                            # IMPGPU_WEBP_MIN_MATCH


def webp_encode_bound(width, height, channels, flags=None):
    """impgpu_webp_encode_bound: a size no lossless WebP file of that frame exceeds (0: a geometry the encoder refuses).
    flags: None = the call itself; a number = impgpu_webp_encode_bound_flags (WEBP_ENC_BACKREFS: backward references)"""
    if flags is None:
        return lib.impgpu_webp_encode_bound(int(width), int(height), int(channels))
    return lib.impgpu_webp_encode_bound_flags(int(width), int(height), int(channels), int(flags))


def _modes(forced_modes):
    return None if forced_modes is None else np.ascontiguousarray(forced_modes, dtype=np.uint8).reshape(-1)


def encode_webp(image, forced_modes=None, capacity=None, guard=64, flags=None):
    """impgpu_image_encode_webp: the image as a lossless WebP file written on the device -> (code, bytes or None, length,
    intact), as encode_gif: `capacity` defaults to webp_encode_bound, `guard` bytes behind it are checked.  forced_modes:
    None = the call itself; one mode 0..13 per tile = impgpu_image_encode_webp_ex (the chooser is skipped).  flags: None =
    those calls; a number = impgpu_image_encode_webp_flags (WEBP_ENC_BACKREFS: backward references, seven launches)."""
    cap = webp_encode_bound(image.shape[1], image.shape[0], image.shape[2], flags) if capacity is None else int(capacity)
    buf = np.full(max(1, cap) + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    if flags is not None:
        keep = _modes(forced_modes)
        rc = lib.impgpu_image_encode_webp_flags(image.h, int(flags), None if keep is None else keep.ctypes.data, buf.ctypes.data, cap, C.byref(n))
    elif forced_modes is None:
        rc = lib.impgpu_image_encode_webp(image.h, buf.ctypes.data, cap, C.byref(n))
    else:
        keep = _modes(forced_modes)
        rc = lib.impgpu_image_encode_webp_ex(image.h, keep.ctypes.data, buf.ctypes.data, cap, C.byref(n))
    return _answer(rc, buf, n)


def encode_webp_host(frame, forced_modes=None, capacity=None, guard=64, channels=None, flags=None):
    """impgpu_webp_encode_host (no device): one HxWxC uint8 array (a view with padded rows is fine) -> (code, bytes or None,
    length, intact), as encode_webp.  flags: None, or impgpu_webp_encode_host_flags'."""
    hh, ww, cc = frame.shape
    assert frame.dtype == np.uint8 and frame.strides[1:] == (cc, 1)
    cc = cc if channels is None else int(channels)
    cap = webp_encode_bound(ww, hh, cc, flags) if capacity is None else int(capacity)
    buf = np.full(max(1, cap) + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    keep = _modes(forced_modes)
    if flags is None:
        rc = lib.impgpu_webp_encode_host(frame.ctypes.data, ww, hh, cc, frame.strides[0], None if keep is None else keep.ctypes.data,
                                         buf.ctypes.data, cap, C.byref(n))
    else:
        rc = lib.impgpu_webp_encode_host_flags(frame.ctypes.data, ww, hh, cc, frame.strides[0], int(flags), None if keep is None else keep.ctypes.data,
                                               buf.ctypes.data, cap, C.byref(n))
    return _answer(rc, buf, n)


def batch_encode_webp(images, capacities=None, count=None, guard=64, flags=None):
    """impgpu_batch_encode_webp: images (an entry may be None) -> (code, [(code, bytes or None, length, intact) ...],
    launches).  capacities default to webp_encode_bound.  flags: None, or impgpu_batch_encode_webp_flags'."""
    n = len(images)
    handles, carr, bufs, outs, lens, codes = _answer_arrays(images, lambda a: webp_encode_bound(a.shape[1], a.shape[0], a.shape[2], flags), capacities, guard)
    launches = C.c_int(-1)
    if flags is None:
        rc = lib.impgpu_batch_encode_webp(handles, n if count is None else count, outs, carr, lens, codes, C.byref(launches))
    else:
        rc = lib.impgpu_batch_encode_webp_flags(handles, n if count is None else count, int(flags), outs, carr, lens, codes, C.byref(launches))
    return rc, [_answer(codes[i], bufs[i], C.c_size_t(lens[i])) for i in range(n)], launches.value


def webp_lossy_encode_bound(width, height, channels):
    """impgpu_webp_lossy_encode_bound: a size no lossy WebP file of that frame exceeds (0: a geometry the encoder refuses)"""
    return lib.impgpu_webp_lossy_encode_bound(int(width), int(height), int(channels))


def encode_webp_lossy(image, quality=75, capacity=None, guard=64):
    """impgpu_image_encode_webp_lossy: the image as a lossy WebP file (VP8 key frame) written on the device -> (code, bytes
    or None, length, intact), as encode_webp: `capacity` defaults to webp_lossy_encode_bound."""
    cap = webp_lossy_encode_bound(image.shape[1], image.shape[0], image.shape[2]) if capacity is None else int(capacity)
    buf = np.full(max(1, cap) + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    rc = lib.impgpu_image_encode_webp_lossy(image.h, int(quality), buf.ctypes.data, cap, C.byref(n))
    return _answer(rc, buf, n)


def encode_webp_lossy_host(frame, quality=75, capacity=None, guard=64, channels=None, details=False):
    """impgpu_webp_lossy_encode_host (no device): one HxWxC uint8 array (a view with padded rows is fine) -> (code, bytes or
    None, length, intact).  details=True: impgpu_webp_lossy_encode_host_ex, and a fifth entry: a dict of the macroblocks'
    modes (n, 2: luma, chroma), levels (n, 25, 16) and the padded reconstructed planes y, u, v."""
    hh, ww, cc = frame.shape
    assert frame.dtype == np.uint8 and frame.strides[1:] == (cc, 1)
    cc = cc if channels is None else int(channels)
    cap = webp_lossy_encode_bound(ww, hh, cc) if capacity is None else int(capacity)
    buf = np.full(max(1, cap) + guard, 0xA5, np.uint8)
    n = C.c_size_t(0)
    if not details:
        rc = lib.impgpu_webp_lossy_encode_host(frame.ctypes.data, ww, hh, cc, frame.strides[0], int(quality), buf.ctypes.data, cap, C.byref(n))
        return _answer(rc, buf, n)
    mw, mh = (max(ww, 1) + 15) // 16, (max(hh, 1) + 15) // 16
    d = {"modes": np.zeros((mw * mh, 2), np.uint8), "levels": np.zeros((mw * mh, 25, 16), np.int16), "y": np.zeros((mh * 16, mw * 16), np.uint8),
         "u": np.zeros((mh * 8, mw * 8), np.uint8), "v": np.zeros((mh * 8, mw * 8), np.uint8)}
    rc = lib.impgpu_webp_lossy_encode_host_ex(frame.ctypes.data, ww, hh, cc, frame.strides[0], int(quality), buf.ctypes.data, cap, C.byref(n),
                                              d["modes"].ctypes.data, d["levels"].ctypes.data, d["y"].ctypes.data, d["u"].ctypes.data, d["v"].ctypes.data)
    return _answer(rc, buf, n) + (d,)


def batch_encode_webp_lossy(images, qualities=None, capacities=None, count=None, guard=64):
    """impgpu_batch_encode_webp_lossy: images (an entry may be None) -> (code, [(code, bytes or None, length, intact) ...],
    launches).  qualities: one per image (default 75); None passes a NULL array.  capacities default to
    webp_lossy_encode_bound."""
    n = len(images)
    handles, carr, bufs, outs, lens, codes = _answer_arrays(images, lambda a: webp_lossy_encode_bound(a.shape[1], a.shape[0], a.shape[2]), capacities, guard)
    launches = C.c_int(-1)
    q = None if qualities is None else (C.c_int * max(1, n))(*[int(v) for v in qualities])
    rc = lib.impgpu_batch_encode_webp_lossy(handles, n if count is None else count, q, outs, carr, lens, codes, C.byref(launches))
    return rc, [_answer(codes[i], bufs[i], C.c_size_t(lens[i])) for i in range(n)], launches.value


def request_webp_quality(uri, extension="", config=None):
    """impgpu_request_webp_quality of the parsed request line: -1, or the lossy WebP quality 0..100 the answer asks for"""
    return Request(uri, extension, config).webp_quality


WEBP_ACCEPT_LOSSY = 1                         # IMPGPU_WEBP_ACCEPT_LOSSY
WEBP_DEC_LOSSY_LAUNCHES = 3                   # IMPGPU_WEBP_DEC_LOSSY_LAUNCHES
WEBP_ACCEPT_ALPHA = 2                         # IMPGPU_WEBP_ACCEPT_ALPHA: with WEBP_ACCEPT_LOSSY, VP8X + ALPH + `VP8 ` files too
WEBP_DEC_ALPHA_LAUNCHES = 1                   # IMPGPU_WEBP_DEC_ALPHA_LAUNCHES


def webp_alpha_info(blob):
    """impgpu_webp_alpha_info -> (code, [method, filter, pre-processing, the VP8L stream's feature word]); host only.
    IMP_ERROR_UNSUPPORTED: no alpha plane that WEBP_ACCEPT_LOSSY | WEBP_ACCEPT_ALPHA would take."""
    b = bytes(blob)
    info = (C.c_int * 4)()
    rc = lib.impgpu_webp_alpha_info(b, len(b), info)
    return rc, list(info)


def webp_info(blob, accept=None):
    """impgpu_webp_info -> (code, width, height, channels); host only.  accept: None = the call itself; a mask =
    impgpu_webp_info_ex (WEBP_ACCEPT_LOSSY: a VP8 key frame's size too; | WEBP_ACCEPT_ALPHA: one with an ALPH chunk)."""
    b = bytes(blob)
    w, h, c = C.c_int(0), C.c_int(0), C.c_int(0)
    if accept is not None:
        rc = lib.impgpu_webp_info_ex(b, len(b), int(accept), C.byref(w), C.byref(h), C.byref(c))
        return rc, w.value, h.value, c.value
    rc = lib.impgpu_webp_info(b, len(b), C.byref(w), C.byref(h), C.byref(c))
    return rc, w.value, h.value, c.value


def webp_decode_host(blob, capacity=None, guard=64, accept=None):
    """impgpu_webp_decode_host (no device): a lossless WebP file -> (code, HxWx4 B,G,R,A array or None, info, intact).
    capacity defaults to what impgpu_webp_info says the frame takes; `intact`: the guard band behind it was not written.
    accept: None = the call itself; a mask = impgpu_webp_decode_host_ex (WEBP_ACCEPT_LOSSY: lossy files too; | WEBP_ACCEPT_ALPHA: their
    alpha planes)."""
    b = bytes(blob)
    rc, w, h, _ = webp_info(b, accept)
    cap = (w * h * 4 if rc == 0 else 0) if capacity is None else int(capacity)
    buf = np.full(max(1, cap) + guard, 0xA5, np.uint8)
    ww, hh = C.c_int(0), C.c_int(0)
    info = (C.c_int * 8)()
    if accept is None:
        rc = lib.impgpu_webp_decode_host(b, len(b), buf.ctypes.data, cap, C.byref(ww), C.byref(hh), info)
    else:
        rc = lib.impgpu_webp_decode_host_ex(b, len(b), int(accept), buf.ctypes.data, cap, C.byref(ww), C.byref(hh), info)
    intact = bool((buf[cap:] == 0xA5).all())
    frame = buf[:ww.value * hh.value * 4].reshape(hh.value, ww.value, 4).copy() if rc == 0 else None
    return rc, frame, list(info), intact


def batch_decode_webp(blobs, count=None, accept=None):
    """impgpu_batch_decode_webp -> ([(code, Image or None)] in the order of `blobs`, kernel launches of the call).
    accept: None = the call itself; a mask = impgpu_batch_decode_webp_ex."""
    n = len(blobs)
    keep = [bytes(b) for b in blobs]
    arr = (C.c_char_p * max(1, n))(*keep)
    sizes = (C.c_size_t * max(1, n))(*[len(b) for b in keep])
    imgs = (C.c_void_p * max(1, n))()
    codes = (C.c_int * max(1, n))()
    launches = C.c_int()
    if accept is None:
        rc = lib.impgpu_batch_decode_webp(arr, sizes, n if count is None else count, imgs, codes, C.byref(launches))
    else:
        rc = lib.impgpu_batch_decode_webp_ex(arr, sizes, n if count is None else count, int(accept), imgs, codes, C.byref(launches))
    if rc:
        raise ImpError(rc, "impgpu_batch_decode_webp")
    return [(codes[i], Image(handle=imgs[i]) if codes[i] == 0 else None) for i in range(n)], launches.value


def decode_webp(blob, accept=None):
    """impgpu_image_decode_webp -> (code, Image or None).  accept: None = the call itself; a mask = impgpu_image_decode_webp_ex."""
    b = bytes(blob)
    h = C.c_void_p()
    if accept is None:
        rc = lib.impgpu_image_decode_webp(b, len(b), C.byref(h))
    else:
        rc = lib.impgpu_image_decode_webp_ex(b, len(b), int(accept), C.byref(h))
    return rc, Image(handle=h.value) if rc == 0 else None


def batch_filters(ptr, stride, w, h, c, step, count, filters, allow_experiments=1, stream=None):
    """Pointwise filter-* requests on every frame of a resident batch, one fused launch. Returns the IMP_* code."""
    arr = (C.c_char_p * max(1, len(filters)))(*[_b(f) for f in filters])
    return lib.impgpu_batch_filters(C.c_void_p(ptr), stride, w, h, c, step, count, arr, len(filters), int(allow_experiments),
                                    C.c_void_p(stream or 0))


class Request:
    """RunJob's parsed request (bridge.c:304-372 + encoder choice :413-466)."""

    def __init__(self, uri, extension="", config=None):
        self.h = C.c_void_p()
        cfg = config or Config()
        self.code = lib.impgpu_parse_request(_b(uri), _b(extension), C.byref(cfg.c), C.byref(self.h))
        j = lib.impgpu_request_job(self.h).contents
        d = lambda v: None if v is None else v.decode()
        self.crop, self.gravity, self.resize = d(j.crop), d(j.gravity), d(j.resize)
        self.simple, self.need_flatten = j.simple, j.need_flatten
        self.filters = [j.filters[i].decode() for i in range(j.filter_count)]
        self.quality = d(lib.impgpu_request_quality(self.h))
        self.format = d(lib.impgpu_request_format(self.h))
        self.page = lib.impgpu_request_page(self.h)
        self.mime = lib.impgpu_request_mime(self.h)
        self.destructive = lib.impgpu_request_destructive(self.h)
        self.webp_lossless = lib.impgpu_request_webp_lossless(self.h)
        self.webp_quality = lib.impgpu_request_webp_quality(self.h)

    def run(self, image, config):
        """impgpu_run_ops with the parsed job. Returns (code, step)."""
        step = C.c_int()
        rc = lib.impgpu_run_ops(C.byref(image.h), lib.impgpu_request_job(self.h), C.byref(config.c), C.byref(step))
        return rc, step.value

    def __del__(self):
        try:
            if self.h:
                lib.impgpu_request_free(C.byref(self.h))
        except Exception:
            pass
