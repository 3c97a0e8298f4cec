/*
 * impgpu.h -- C ABI of libimpgpu.so: the MI355X (gfx950) pixel-transform path that
 * replaces the operator segment of IMP's RunJob (reference bridge.c:574-656) and the
 * OpenCV/filters.c calls below it.  Plain C types only; no torch, no C++ in signatures.
 *
 * Each entry point cites the reference interface it stands in for.  Argument strings
 * are the reference's GET-parameter values verbatim (docs/03 - Usage.md); return codes
 * are the reference's IMP_* codes (required.h:28-41).  All pixel work runs in HIP
 * kernels on the device selected by impgpu_env_start(); there is no CPU fallback --
 * every device-touching call returns IMP_ERROR_DEVICE when HIP is unavailable.
 *
 * Images are 8-bit interleaved B,G,R[,A] (required.h:66-69), top-left origin, rows
 * padded to 4 bytes exactly like cvCreateImage (widthStep = (w*channels + 3) & ~3).
 */
#ifndef IMPGPU_H
#define IMPGPU_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: required.h:28-41 ---- */
#define IMP_OK                      0
#define IMP_ERROR_UNSUPPORTED       1
#define IMP_ERROR_MALLOC_FAILED     2
#define IMP_ERROR_DECODE_FAILED     3
#define IMP_ERROR_ENCODE_FAILED     4
#define IMP_ERROR_INVALID_ARGS      50
#define IMP_ERROR_UPSCALE           51
#define IMP_ERROR_NO_SUCH_FILTER    52
#define IMP_ERROR_NO_SUCH_WATERMARK 53
#define IMP_ERROR_TOO_BIG_TARGET    54
#define IMP_ERROR_TOO_MUCH_FILTERS  55
#define IMP_ERROR_FEATURE_DISABLED  56
/* not in the reference: a HIP runtime call failed or no device/env (maps to HTTP 500 like any other code) */
#define IMP_ERROR_DEVICE            90

/* ---- step codes: required.h:46-54 ---- */
#define IMP_STEP_START     0
#define IMP_STEP_VALIDATE  1
#define IMP_STEP_DECODE    2
#define IMP_STEP_CROP      3
#define IMP_STEP_RESIZE    4
#define IMP_STEP_FILTERING 5
#define IMP_STEP_WATERMARK 6
#define IMP_STEP_INFO      7
#define IMP_STEP_ENCODE    8

/* ---- interpolation ids: OpenCV 2.4 CV_INTER_* as passed to cvResize at bridge.c:190-191 ---- */
#define IMP_INTER_NN       0
#define IMP_INTER_LINEAR   1
#define IMP_INTER_CUBIC    2
#define IMP_INTER_AREA     3
#define IMP_INTER_LANCZOS4 4

/* Device-resident stand-in for the IplImage* the reference passes between operators
 * (required.h:129-134 Frame.Image). Opaque; query with the accessors. */
typedef struct impgpu_image impgpu_image;

/* The fields of Config (required.h:108-118) that the operators read, plus Position
 * (required.h:86-91).  watermark replaces RecoverInfo (required.h:99-106): the overlay's
 * pixels live in HBM, uploaded once per worker by impgpu_prepare_watermark. */
typedef struct {
    unsigned int  max_target_w;         /* MaxTargetDimensions->W, 0 = unlimited (module.c:172-175 default 2000) */
    unsigned int  max_target_h;         /* MaxTargetDimensions->H */
    int           max_filters_count;    /* MaxFiltersCount (module.c:181 default 5) */
    int           allow_experiments;    /* AllowExperiments */
    int           watermark_opacity;    /* WatermarkOpacity 1..100 (module.c:144-148) */
    char          watermark_gravity_x;  /* Position.GravityX: 'l' 'c' 'r' */
    char          watermark_gravity_y;  /* Position.GravityY: 't' 'c' 'b' */
    int           watermark_offset_x;   /* Position.OffsetX */
    int           watermark_offset_y;   /* Position.OffsetY */
    impgpu_image* watermark;            /* WatermarkInfo; NULL = no watermark configured */
} impgpu_config;

/* What RunJob has parsed out of the query string by bridge.c:372, i.e. the inputs of
 * the operator segment bridge.c:574-656. */
typedef struct {
    const char*        crop;            /* value of crop=, NULL if absent */
    const char*        gravity;         /* value of gravity=, NULL if absent */
    const char*        resize;          /* value of resize=, NULL if absent */
    int                simple;          /* bridge.c:594: GIF output forces nearest-neighbour */
    const char* const* filters;         /* "name=args" strings in query order (bridge.c:365) */
    int                filter_count;
    int                need_flatten;    /* encoder lacks alpha (bridge.c:642-648) */
} impgpu_job;

/* ---- lifecycle: OnEnvStart / OnEnvDestroy (bridge.h:1-2, bridge.c:10-16; called from
 *      module.c:100-107 once per worker process, after fork) ---- */
/* device < 0: take $IMPGPU_DEVICE, else $LOCAL_RANK, else 0.
 * impgpu_env_start also registers impgpu_env_destroy with atexit() (once per process): a worker that leaves through
 * exit() with a live env gives its streams, events, pinned buffers and pool blocks back BEFORE the HIP runtime's own exit
 * handlers run, not during them.  That exit-time teardown waits at most $IMPGPU_EXIT_WAIT_MS (default 2000) for the
 * device to go idle and otherwise leaves everything to the driver; a fork()ed copy of a process that started the env
 * does nothing at exit.  impgpu_env_destroy is idempotent. */
int         impgpu_env_start(int device);
void        impgpu_env_destroy(void);
int         impgpu_env_device(void);            /* -1 when no env */
/* NUMA: the node the env's device hangs off (its PCI function's numa_node; -1 = unknown or a one-node
 * host), and a call that binds the CALLING thread to that node's CPUs -- a worker's staging copies then run next to
 * the GPU's PCIe root, and pinned memory the thread allocates afterwards is that node's (first touch).  An nginx worker
 * calls it once after impgpu_env_start; IMPGPU_NUMA_BIND=1 does it for every thread at its first call into the library.
 * IMP_ERROR_UNSUPPORTED when the node is unknown or none of its CPUs is open to this process. */
int         impgpu_env_numa_node(void);
int         impgpu_env_bind_thread(void);
const char* impgpu_last_error(void);            /* text of the last HIP failure on this thread */
int         impgpu_sync(void);                  /* wait for the env stream */
void*       impgpu_env_stream(void);            /* the env's hipStream_t */

/* Test hook (failure detection): the nth entry (1 = the next) into the given IMP_STEP_* behaves as if its first
 * HIP call had failed -- IMP_ERROR_DEVICE, impgpu_last_error() says "injected fault", the failing step is reported like
 * any other -- so the path a lost device takes can be tested without losing one.  step < 0 disarms.  Armed by this call
 * only, never by the environment. */
int         impgpu_fault_arm(int step, long nth);

/* ---- frames: the decode -> operators hand-over (bridge.c:547-552, advancedio.c:310-318)
 *      and the operators -> encode hand-over (bridge.c:703-704, advancedio.c:65-101) ---- */
int   impgpu_image_upload(const unsigned char* data, int width, int height, int channels,
                          int step, impgpu_image** out);   /* pinned staging + hipMemcpyAsync */
int   impgpu_image_create(int width, int height, int channels, impgpu_image** out);
/* Pinned-host variants for callers that decode into / encode from page-locked memory
 * (impgpu_host_alloc): no staging pass, fully asynchronous on the env stream.  The host
 * buffer must stay untouched until impgpu_sync() (upload) / is valid after impgpu_sync() (download).
 * `step` may be any host row pitch >= width * channels: a pitch other than the frame's own (4-byte padded rows) still
 * crosses the link as one linear copy and is re-pitched on the device; on download the bytes between the caller's rows
 * are then written as zeros. */
void* impgpu_host_alloc(size_t bytes);
void  impgpu_host_free(void* ptr);
int   impgpu_image_upload_pinned(const unsigned char* data, int width, int height, int channels,
                                 int step, impgpu_image** out);
int   impgpu_image_download_pinned(const impgpu_image* image, unsigned char* data, int step);
/* The FreeImage side of the hand-overs (advancedio.c): bitmaps there are bottom-up with 4-byte aligned rows.
 * upload_fi32 = LoadSingle's copy loop (advancedio.c:310-318): 32-bit bits -> 4-channel top-down frame.
 * download_fi = IplToFI32 / IplToFI24 (advancedio.c:65-101): flip, and B,G,R,A with A = 255 for 3-channel frames
 * (bpp 32) or B,G,R with alpha dropped (bpp 24), written into the encoder's bitmap; the repack runs on the device. */
int   impgpu_image_upload_fi32(const unsigned char* bits, int width, int height, int pitch, impgpu_image** out);
int   impgpu_image_download_fi(const impgpu_image* image, int bpp, unsigned char* bits, int pitch);   /* syncs */
/* download_fi for every frame of an album (SaveGIF's per-frame IplToFI32, advancedio.c:350): frame i into bits[i] with
 * pitches[i] bytes per row; all repacks and the copy are enqueued, then ONE wait.  A single image is an album of one. */
int   impgpu_album_download_fi(const impgpu_image* album, int bpp, unsigned char* const* bits, const int* pitches);
/* impgpu_album_download_fi for `count` handles (0..256; albums and single images mixed) behind ONE wait.
 * bits[] / pitches[] have one entry per FRAME: handle 0's frames first, in frame order, then handle 1's ...
 * (sum of impgpu_album_count).  bpps[i] is 24 or 32 per handle.  Every frame of the call is flipped and repacked into one
 * device block by ONE launch per (source channels, bpp) pair present -- at most four, one when the call is uniform;
 * *launches (may be NULL) receives the number -- then one copy into pinned staging and one wait (a call whose bitmaps
 * pass $IMPGPU_STAGE_CAP_MB is cut at a handle into groups in handle order, each with its own copy and wait).  An entry
 * impgpu_album_download_fi refuses (a NULL handle, which owns no entries of bits[]; fewer than 3 channels; a bpp other
 * than 24 or 32; a NULL bits entry; a pitch below width * bpp / 8) gets IMP_ERROR_INVALID_ARGS in codes[i] alone and
 * nothing of it is touched.  Returns IMP_ERROR_INVALID_ARGS for NULL arrays with count > 0 or a count outside 0..256
 * (before any device is looked for; count = 0 is IMP_OK there too), IMP_ERROR_DEVICE without an env (every codes[i] says so too), otherwise IMP_OK with
 * the verdicts in codes[].  Only the first width * bpp / 8 bytes of each of the caller's rows are written. */
int   impgpu_batch_download_fi(const impgpu_image* const* images, const int* bpps, int count,
                               unsigned char* const* bits, const int* pitches, int* codes, int* launches);
/* The decode itself moved in front of the operators: IplImage* image = cvDecodeImage(&rawencoded, -1)   bridge.c:545-552
 * for a JPEG blob (SIG_JPG, bridge.c:376-378), i.e. libjpeg with its default parameters (ISLOW IDCT, fancy upsampling)
 * and OpenCV's R/B swap.  The compressed bytes cross the link instead of the pixels; Huffman decoding, dequantisation,
 * IDCT, chroma upsampling and YCbCr -> B,G,R run on the device and the frame (3 channels, or 1 for a gray file, exactly
 * what cvDecodeImage(.., -1) returns) is bit-identical to libjpeg-turbo's.  Takes 8-bit baseline / extended-sequential
 * Huffman files with one interleaved scan and 4:4:4, 4:2:2, 4:4:0, 4:2:0 or gray sampling, with or without restart
 * intervals.  IMP_ERROR_UNSUPPORTED = a JPEG outside that set (progressive, CMYK, ...): decode it with cvDecodeImage as
 * before and impgpu_image_upload the pixels.  IMP_ERROR_DECODE_FAILED = damaged data; libjpeg would warn and deliver
 * what it could, so the same fallback applies.  Waits for the device's verdict on the entropy-coded data before it
 * returns (the only wait on the request path besides the download).  A launch with less than 40 KB of entropy-coded
 * data keeps its Huffman decoding on the calling thread (6 ns per byte against a fixed few hundred microseconds of
 * device rounds); IMPGPU_JPEG_HUFF=device|host forces one.  The pixels do not depend on it. */
int   impgpu_image_decode_jpeg(const unsigned char* blob, size_t size, impgpu_image** out);
/* The same for `count` files at once -- the frames of a request queue (BASELINE configs[4]) or whatever else arrives
 * together: ONE entropy launch and one pixel launch per chroma sampling for all of them, one wait for all verdicts, so the
 * device is filled by a single caller.  codes[i] / images[i] are what impgpu_image_decode_jpeg would return for file i
 * (images[i] = NULL unless codes[i] == IMP_OK); the return value is IMP_OK unless the call itself failed (no env, a HIP
 * error), in which case no image is returned. */
int   impgpu_batch_decode_jpeg(const unsigned char* const* blobs, const size_t* sizes, int count,
                               impgpu_image** images, int* codes);
/* The same in two halves, for a caller that has more to do than wait (round 4): _begin parses, copies the scans into pinned
 * memory and enqueues the whole decode -- it does NOT wait; _finish sleeps until THAT batch is done (not whatever the thread
 * enqueued after it), reads the verdicts and fills images[] / codes[] as impgpu_batch_decode_jpeg would.  Between the two the
 * thread may begin the next batch or enqueue anything else; the blobs must stay readable until _finish (a file the device
 * defers is read again).  Both halves belong to ONE thread: _finish from another thread returns IMP_ERROR_INVALID_ARGS and
 * leaves the batch with its owner.  A thread has FOUR slots for decodes in flight, shared by the batches it has begun and
 * by its ordinary decode calls (one each; a one-call batch of 32 or more files takes two when two are free): with four
 * batches begun and not finished, any further decode on that thread returns IMP_ERROR_INVALID_ARGS.  count <= 256.
 * The batch runs on a second stream of the calling thread, so work the thread enqueues between the two calls (the resize and
 * the answers of the batch before) overlaps it.  (impgpu_batch_decode_jpeg itself already prepares the second half of a large
 * batch while the device works on the first; profiles/r05_jpeg_stream_native.txt holds both forms side by side.) */
typedef struct impgpu_jpeg_batch impgpu_jpeg_batch;
int   impgpu_batch_decode_jpeg_begin(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_jpeg_batch** batch);
int   impgpu_batch_decode_jpeg_finish(impgpu_jpeg_batch** batch, impgpu_image** images, int* codes);
/* Files whose entropy-coded segment has been taken out of its byte stuffing by the CALLER (round 5: a worker process does it
 * while it copies its request into the broker's shared memory -- impgpu_jpeg_unstuff in libimpgpu_client.so -- so the pass over
 * the compressed bytes is made by sixteen sleeping workers instead of the four threads that drive the device).
 *   head, head_size   the file from SOI up to and including its SOS header (what jpeg headers parse); a file WITH a restart
 *                     interval cannot be handed over this way (IMP_ERROR_INVALID_ARGS for that file);
 *   scan, scan_size   the entropy-coded bytes that followed, FF 00 -> FF, fill bytes dropped, up to (not including) the marker
 *                     that ends them; behind them the caller has written IMPGPU_JPEG_SCAN_TAIL bytes of 0xFF (not counted);
 *                     scan = NULL: `head` is a whole file as it came (the two kinds may share a batch);
 *   registered        != 0: `scan` lies in memory made known with impgpu_host_register -- the bytes go to the device from
 *                     where they are (no pass over them on the calling thread at all); they must not change until the call
 *                     returns.
 * Pixels, codes and refusals are those of impgpu_batch_decode_jpeg on the original files. */
#define IMPGPU_JPEG_SCAN_TAIL 1024
typedef struct {
    const unsigned char* head; size_t head_size;
    const unsigned char* scan; size_t scan_size;
    int registered;
} impgpu_jpeg_prepared;
int   impgpu_batch_decode_jpeg_prepared(const impgpu_jpeg_prepared* files, int count, impgpu_image** images, int* codes);
/* ... and in two halves like impgpu_batch_decode_jpeg_begin, but on the calling thread's OWN stream: what the thread enqueues
 * afterwards runs behind this decode, what it enqueued before runs in front of it (a broker lane begins the next batch's
 * decode while the answers of the batch before are still being written: the device never waits for the host's share).
 * The array is copied; head / scan bytes must stay readable until impgpu_batch_decode_jpeg_finish.  count <= 256. */
int   impgpu_batch_decode_jpeg_prepared_begin(const impgpu_jpeg_prepared* files, int count, impgpu_jpeg_batch** batch);
/* The frames of a batch begun on the calling thread's own stream (impgpu_batch_decode_jpeg_prepared_begin), AHEAD of their verdicts:
 * images[i] = the frame file i is being decoded into -- geometry final, pixels there once the batch's kernels have run, which is
 * before anything the thread enqueues on it afterwards runs -- or NULL where there is none yet (refused at its header, or a file
 * whose Huffman stage the host keeps: those come out of _finish as before).  Ownership passes to the caller; _finish then
 * returns NULL for that file and its CODE: not IMP_OK = the frame does not hold the file's pixels (release it, or whatever was
 * made of it, and fall back like for any refused file).  So a request's operators and its answer's encode can be enqueued
 * BEHIND the decode and the thread waits once, at the end, instead of once for the verdicts and once for the answer: a lone
 * 640 x 480 -> thumbnail -> JPEG request 0.29 -> see DESIGN 4b. */
int   impgpu_batch_decode_jpeg_pending(impgpu_jpeg_batch* batch, impgpu_image** images);
/* Page-locks `bytes` at `p` (hipHostRegister) so that copies out of it need no staging; impgpu_host_unregister before the
 * memory goes away.  Needs impgpu_env_start. */
int   impgpu_host_register(void* p, size_t bytes);
int   impgpu_host_unregister(void* p);
/* Where a decode call's time goes (per-stage timing): impgpu_jpeg_profile(1) makes every later decode call leave
 * its stages with the calling thread, impgpu_jpeg_stage_times reads the last call's, in microseconds:
 * [0] marker segments, [1] FF00 unstuffing into pinned memory, [2] tables + job table, [3] enqueue, [4] wait for the verdicts
 * (host clock); [5] upload, [6] k_jpeg_walks, [7] k_jpeg_mend, [8] k_jpeg_select, [9] k_jpeg_write, [10] k_jpeg_dcfix,
 * [11] verdict copy + k_jpeg_pixels (events on the stream; the call then also waits for the pixels); [12] files decoded.
 * Returns the previous setting / IMP_OK. */
int   impgpu_jpeg_profile(int on);
/* Process-wide counts since the library was loaded: [0] files whose entropy stage ran on the device, [1] of those, refused
 * by its verdict (the caller's cvDecodeImage fallback took them), [2] of those, because a wait between workgroups ran out --
 * must stay 0 on a healthy box, however many processes share the device -- [3] files kept on the calling thread because
 * their blocks are too long for the device scheme (more than 200 bits each).
 * Round 5, what the cvDecodeImage fallback (bridge.c:545-552) is paid for -- files a decode call refused at their header, by
 * reason: [5] progressive (SOF2), [6] arithmetic / lossless / hierarchical, [7] 12-bit samples, [8] CMYK / YCCK or another
 * component count, [9] not one interleaved scan, [10] sampling factors outside 1x1 / 2x1 / 1x2 / 2x2 over 1x1, [11] anything
 * else (a DNL height, not a JPEG at all), [12] headers damaged before the first scan.  ([4] is unused.)
 * impgpu_jpeg_classify gives the same verdict for one file without decoding it (host, no device): 0 = the device takes it,
 * 1..7 = the reasons in the order above, 8 = damaged; tools/corpus_probe.py adds them up over a directory. */
int   impgpu_jpeg_counters(unsigned long long* counters, int n);
int   impgpu_jpeg_classify(const unsigned char* blob, size_t size);
int   impgpu_jpeg_stage_times(double* microseconds, int n);
/* The other end of the request: CvMat* encoded = cvEncodeImage(".jpg", image, basicCoderopt)          bridge.c:704
 * with basicCoderopt = {CV_IMWRITE_JPEG_QUALITY, quality} (bridge.c:474-486; OpenCV clamps the value to 0..100), for the
 * frame the operators left in HBM: colour conversion, chroma downsampling, forward DCT, quantisation and Huffman coding run
 * on the device and the compressed file crosses the link instead of the pixels.  OpenCV 2.4.9's JpegEncoder leaves
 * everything else at libjpeg's defaults -- baseline, YCbCr 4:2:0 (one gray component for a 1-channel frame), the Annex K
 * tables, ISLOW DCT, JFIF 1.01 -- and the file is the same, byte for byte, as libjpeg-turbo's.  A 4-channel frame loses
 * its alpha exactly as in cvEncodeImage (RunJob flattens it first, bridge.c:642-656); an album handle encodes frame 0,
 * like bridge.c:703.  *length receives the file's size; IMP_ERROR_MALLOC_FAILED = capacity is smaller than that (nothing
 * is written; impgpu_jpeg_encode_bound(w, h, c) is always enough).  Waits for the device. */
int   impgpu_image_encode_jpeg(const impgpu_image* image, int quality, unsigned char* out, size_t capacity, size_t* length);
/* `count` frames (the thumbnails of a request queue) in two launches and two waits; codes[i] / lengths[i] are what
 * impgpu_image_encode_jpeg would give for frame i. */
int   impgpu_batch_encode_jpeg(const impgpu_image* const* images, int count, int quality, unsigned char* const* outs,
                               const size_t* capacities, size_t* lengths, int* codes);
/* The same in two halves (round 5, for a caller that serves more than one batch: a broker lane): _begin enqueues everything --
 * kernels and the copy of the files' segments into pinned memory -- and does NOT wait; _finish sleeps until THAT encode is
 * done (not what the thread enqueued behind it, e.g. the decode of the next batch), and fills outs[] / lengths[] / codes[] as
 * impgpu_batch_encode_jpeg would.  The frames must stay alive until _finish.  Both halves belong to ONE thread.  The answers
 * of an encode wait in one of the thread's TWO pinned staging buffers until they are fetched: with two encodes begun, anything
 * else of that thread that stages through pinned memory (a third encode, a decode, an upload) returns IMP_ERROR_INVALID_ARGS
 * until one is finished -- a lane keeps one in flight.  count <= 256. */
typedef struct impgpu_jpeg_encode impgpu_jpeg_encode;
int   impgpu_batch_encode_jpeg_begin(const impgpu_image* const* images, int count, int quality, impgpu_jpeg_encode** encode);
int   impgpu_batch_encode_jpeg_finish(impgpu_jpeg_encode** encode, unsigned char* const* outs, const size_t* capacities,
                                      size_t* lengths, int* codes);
size_t impgpu_jpeg_encode_bound(int width, int height, int channels);
/* The PNG answer: CvMat* encoded = cvEncodeImage(".png", image, basicCoderopt)                         bridge.c:704
 * with basicCoderopt = {CV_IMWRITE_PNG_COMPRESSION, level} (bridge.c:487-497; quality= in 0..9, 9 when absent), for the
 * frame the operators left in HBM: the row filters, the deflate symbols, the Huffman trees and the bit stream are made on
 * the device and the compressed file crosses the link instead of the pixels.  OpenCV 2.4.9's PngEncoder asks libpng for
 * strategy Z_RLE, libpng's own filter choice, png_set_bgr, 8-bit gray / RGB / RGBA (1 / 3 / 4 channels), no interlace,
 * no chunks besides IHDR, IDAT, IEND -- and the file is the same, byte for byte, as libpng 1.6.37 over zlib 1.2.11's.
 * Under Z_RLE levels 1..9 give the same file.  A 4-channel frame keeps its alpha (RunJob flattens only for JPEG); an album
 * handle encodes frame 0, like bridge.c:703; a view with step > width * channels is fine.  IMP_ERROR_UNSUPPORTED = level 0
 * (stored blocks whose sizes depend on how libpng feeds zlib), a 2-channel frame, a width or height above 1 000 000 (libpng's
 * write limits: cvEncodeImage fails there too) or more than 2^28 bytes of filtered rows: encode it with cvEncodeImage as before.  IMP_ERROR_INVALID_ARGS = any other level outside 1..9.  *length receives the
 * file's size; IMP_ERROR_MALLOC_FAILED = capacity is smaller than that (nothing is written; impgpu_png_encode_bound(w, h, c)
 * is always enough, stored blocks included).  Waits for the device. */
int   impgpu_image_encode_png(const impgpu_image* image, int level, unsigned char* out, size_t capacity, size_t* length);
/* `count` frames (count <= 256; any sizes and channel counts mixed) in one set of launches and two waits; codes[i] /
 * lengths[i] are what impgpu_image_encode_png would give for frame i. */
int   impgpu_batch_encode_png(const impgpu_image* const* images, int count, int level, unsigned char* const* outs,
                              const size_t* capacities, size_t* lengths, int* codes);
size_t impgpu_png_encode_bound(int width, int height, int channels);
/* Diagnostic (host, no device): the zlib stream libpng would write for `size` bytes of filtered scanlines, made by the
 * device's own symbol / tree / bit code (csrc/imp_png_deflate.h) run on one host thread.  *length = the stream's size;
 * IMP_ERROR_MALLOC_FAILED when capacity is smaller. */
int   impgpu_png_deflate(const unsigned char* data, size_t size, unsigned char* out, size_t capacity, size_t* length);
/* the SOF header alone (host, no device): the size checks the module makes before decoding */
int   impgpu_jpeg_info(const unsigned char* blob, size_t size, int* width, int* height, int* channels);
/* Diagnostics (host, no device): the quantised coefficients of the file's components, MCU-padded planes one after the
 * other, blocks in raster order, 64 shorts each in row-major order.  how = 0: a plain sequential entropy decoder;
 * how = 1: the device's chunk-parallel scheme executed lane by lane on the host (same code as the kernel's lanes).
 * info[0] = shorts written, [1] = the scheme's status word, [2] = chunks whose true entry state was not among their
 * walks' (how = 1), [3..5] = first short of each component's plane, [6..8] / [9..11] = blocks per row / column.
 * impgpu_jpeg_sync_stats: more about the calling thread's last how = 1 call -- stats[0] = chunks, [1] = the same misses,
 * [2] = repair walks (speculative ones included), [3] = chunks reached by an explicit state ("chase"), [4] = chunk bits,
 * [5] = overlap bits, [6] = walks per chunk. */
int   impgpu_jpeg_coefficients(const unsigned char* blob, size_t size, int how, short* out, size_t capacity, int* info);
void  impgpu_jpeg_sync_stats(int stats[8]);
/* ---- progressive JPEG in (opt-in: nothing changes for a caller who does not ask) ----
 * The calls above with an `accept` mask.  accept == 0: the old call's answers, codes and launch counts.  With
 * IMPGPU_JPEG_PROGRESSIVE a call also takes SOF2 files: 8-bit, 1 or 3 components, the sampling factors the sequential path
 * takes, up to 32 scans in any legal order (libjpeg's default script has 10, mozjpeg's 9 to 12) -- DC scans interleaved or
 * not, AC scans, spectral selection, successive approximation, DHT and DRI segments between scans, restart intervals.  A
 * complete progressive file holds the coefficients of its sequential twin and libjpeg makes the same pixels of them, so
 * the frame is bit-identical to libjpeg-turbo's here too.
 * IMP_ERROR_UNSUPPORTED, at the header (decode with cvDecodeImage as before): a scan script after which some coefficient
 * has not been sent down to Al = 0 (libjpeg would smooth, or show a coarse image); a progression T.81 G.1.1.1.1 forbids (AC
 * before DC, a refinement whose Ah is not the previous Al, a band sent twice, an AC scan of several components, Ss / Se out
 * of range: libjpeg only warns); more than 32 scans; a DQT segment behind the first scan.  IMP_ERROR_DECODE_FAILED: damaged
 * entropy data (a code that is not in the table, an interval that runs out of bits or has a byte or more left over, a wrong
 * RSTn, no EOI), found on the device per file -- a bad file changes no other file's result.
 * How it runs: the host walks the markers and unstuffs every scan into the call's one upload; the device zeroes the
 * planes, then decodes (file, scan, restart interval) items, one launch per LEVEL for the whole call -- a scan's level is
 * 1 + the highest level of an earlier scan that touches the same component and an overlapping band; libjpeg's ten-scan
 * script has three -- so the launches follow the deepest script of the batch, not the number of files; then the same
 * pixel kernels as for sequential files.  (impgpu_batch_decode_jpeg_ex cuts a batch of 32 files or more into two groups
 * like impgpu_batch_decode_jpeg does: each group has its own launches.)  There is no parallelism INSIDE an interval: a
 * lone large file without restart intervals has a handful of items per level and is decoded by as many lanes.
 * MEASURED (profiles/jpeg_prog_probe.json): that loses to the host.  A lone 640 x 480 / 1080p / 4K progressive
 * photograph takes 0.30 / 2.1 / 8.3 s here against 3.2 / 21 / 103 ms for libjpeg-turbo on one core plus
 * impgpu_image_upload, and a batch of 64 still 10 / 67 ms per file against those 3.2 / 21: a lane decodes about 0.3 MB/s.
 * Until a scan is decoded by many lanes (not built) keep progressive files on the host unless moving the work off the
 * host's cores is worth that latency; the call does not switch by size on its own.
 * _finish and _pending serve batches begun either way; _pending returns the frame of a progressive file like any other's
 * (it is NULL only where the old call's is).  In _prepared_begin_ex a progressive file comes whole: head = the file,
 * scan == NULL (impgpu_jpeg_unstuff passes such a file on whole).  impgpu_jpeg_classify keeps answering 1 for SOF2: it
 * names a kind, not a refusal.  impgpu_jpeg_counters [13] = progressive files decoded on the device, [14] = level
 * launches made for them ([5] keeps counting the progressive files REFUSED).  impgpu_jpeg_stage_times [13] = the zero fill
 * and the level launches of the call's last group in microseconds (events), [14] = how many level launches, [15] = its
 * progressive files.
 * impgpu_jpeg_coefficients_ex (host, no device): how = 0 a plain bit-by-bit decoder of the file as it is; how = 1 the
 * device's items run one after the other on the host by the lanes' own code; info[2] = the script's levels. */
#define IMPGPU_JPEG_PROGRESSIVE 1
int   impgpu_image_decode_jpeg_ex(const unsigned char* blob, size_t size, int accept, impgpu_image** out);
int   impgpu_batch_decode_jpeg_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept,
                                  impgpu_image** images, int* codes);
int   impgpu_batch_decode_jpeg_begin_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept,
                                        impgpu_jpeg_batch** batch);
int   impgpu_batch_decode_jpeg_prepared_begin_ex(const impgpu_jpeg_prepared* files, int count, int accept, impgpu_jpeg_batch** batch);
int   impgpu_jpeg_info_ex(const unsigned char* blob, size_t size, int accept, int* width, int* height, int* channels);
int   impgpu_jpeg_coefficients_ex(const unsigned char* blob, size_t size, int how, int accept, short* out, size_t capacity, int* info);
/* ---- PNG in (round 4, a bounded experiment: DESIGN.md "PNG decode") ----
 * cvDecodeImage(&rawencoded, -1) (bridge.c:545-552) for a PNG blob (SIG_PNG, bridge.c:376-378), i.e. OpenCV 2.4's PngDecoder
 * over libpng with the "unchanged" flag: 8-bit gray -> 1 channel, RGB -> BGR, RGBA -> BGRA, tRNS not expanded.  The zlib
 * stream is inflated on the HOST (csrc/imp_inflate.cpp) straight into pinned memory; the filtered scanlines cross the link and the five
 * scanline filters (PNG specification 9.2) are undone on the device.  Takes bit depth 8, colour types 0 / 2 / 6, not
 * interlaced, width <= 4096, height <= 16384; IMP_ERROR_UNSUPPORTED = any other PNG (or not a PNG): decode it with
 * cvDecodeImage as before.  IMP_ERROR_DECODE_FAILED = damaged (a chunk's CRC, the deflate stream, too little data, a
 * filter type above 4; the stream's Adler-32 trailer is not checked).  Does not wait for the device.
 * impgpu_png_stage_times: the calling thread's last decode, host clock, microseconds: [0] header, [1] chunk walk + CRC +
 * inflate, [2] filter-type check + enqueue (upload, kernel); [3] = bytes of filtered scanlines. */
int   impgpu_image_decode_png(const unsigned char* blob, size_t size, impgpu_image** out);
/* Many PNG files in one call (count <= 256): codes[i] / images[i] are what impgpu_image_decode_png(blobs[i], sizes[i]) returns
 * alone -- the same pixels, refusals and damage verdicts; a refused or damaged file changes no other file's result.  The headers
 * are read on the calling thread, the accepted files are inflated side by side (the helper threads the JPEG batch uses) into
 * one pinned buffer, uploaded once, and ONE k_png_unfilter_batch launch per channel count present (1 / 3 / 4) unfilters them,
 * a workgroup per file.  Files whose scanlines together exceed IMPGPU_STAGE_CAP_MB go in groups, in file order, each of
 * its own upload and launches.  *launches (may be NULL) = the kernels the call launched: no copy or fill kernels, so at most
 * one per channel count and group.  The blobs are not read after the call returns; it does not wait for the device.
 * IMP_ERROR_INVALID_ARGS = a NULL array or count outside 0..256 (before any device is looked for); IMP_ERROR_DEVICE =
 * impgpu_env_start has not been called.  impgpu_png_stage_times keeps describing the thread's last single-file decode. */
int   impgpu_batch_decode_png(const unsigned char* const* blobs, const size_t* sizes, int count,
                              impgpu_image** images, int* codes, int* launches);
int   impgpu_png_info(const unsigned char* blob, size_t size, int* width, int* height, int* channels);
int   impgpu_png_stage_times(double* microseconds, int n);
/* Diagnostics (host, no device): the filtered scanlines of the file -- height rows of (1 filter byte + width * channels bytes),
 * as the device receives them -- after the chunk walk, the CRC checks and the inflate.  *length = the bytes the image needs
 * (set whenever the header was readable); IMP_ERROR_MALLOC_FAILED when capacity is smaller. */
int   impgpu_png_scanlines(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, size_t* length);
/* ---- PNG in, more kinds (opt-in: DESIGN.md "PNG decode", items and passes) ----
 * The calls above with an `accept` mask of further kinds, each decoded as cvDecodeImage(blob, -1) over libpng 1.6 gives it:
 *   IMPGPU_PNG_PALETTE   colour type 3, depth 1 / 2 / 4 / 8, no tRNS -> 3 channels, B,G,R from PLTE; an index past the
 *                        PLTE's entries gives (0, 0, 0)
 *   IMPGPU_PNG_LOW_GRAY  colour type 0, depth 1 / 2 / 4 -> 1 channel, samples scaled by 255 / 85 / 17 (tRNS not expanded)
 *   IMPGPU_PNG_ADAM7     interlaced files of every kind otherwise taken (today's 8-bit gray / RGB / RGBA included): the
 *                        pixels of the same image not interlaced
 * A kind outside the mask is refused exactly as the call without _ex refuses it, and accept == 0 gives that call's answers.
 * Still IMP_ERROR_UNSUPPORTED: palette with tRNS, gray + alpha, 16-bit, a PLTE of more than 2^depth entries, width > 4096
 * or height > 16384.  IMP_ERROR_DECODE_FAILED besides the usual damage: a palette file without one PLTE before its IDAT, or
 * with an empty PLTE, one longer than 768 bytes or not a multiple of 3; an Adam7 stream too short for its passes.
 * Files of today's kinds that are not interlaced go the way they go without _ex (a lone file streams its rows); the others
 * are inflated on the host, each non-empty pass (or the whole file) is unfiltered by k_png_unfilter_batch as an item of its
 * own, and k_png_place writes the answer's pixels: one launch per channel count for the whole call. */
#define IMPGPU_PNG_PALETTE  1
#define IMPGPU_PNG_LOW_GRAY 2
#define IMPGPU_PNG_ADAM7    4
#define IMPGPU_PNG_ALL      (IMPGPU_PNG_PALETTE | IMPGPU_PNG_LOW_GRAY | IMPGPU_PNG_ADAM7)
int   impgpu_image_decode_png_ex(const unsigned char* blob, size_t size, int accept, impgpu_image** out);
int   impgpu_batch_decode_png_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept,
                                 impgpu_image** images, int* codes, int* launches);
int   impgpu_png_info_ex(const unsigned char* blob, size_t size, int accept, int* width, int* height, int* channels);
/* Diagnostic (host, no device): the filtered bytes of every non-empty pass in pass order (one item when not interlaced), each
 * pass's rows of (1 filter byte + ceil(pass width * bits per pixel / 8) bytes).  *length as impgpu_png_scanlines. */
int   impgpu_png_scanlines_ex(const unsigned char* blob, size_t size, int accept, unsigned char* out, size_t capacity, size_t* length);
/* ---- PNG in, inflated on the device (opt-in: DESIGN.md "PNG decode", the device inflate) ----
 * IMPGPU_PNG_DEVICE_INFLATE is a further bit of `accept`, NOT part of IMPGPU_PNG_ALL.  It selects HOW files are decoded, not
 * WHICH: codes[i] / images[i] are what the same call without the bit gives -- the same pixels, refusals and damage verdicts.
 * impgpu_batch_decode_png_ex with the bit: the host still reads the headers, walks the chunks, checks every CRC and gathers
 * each accepted file's IDAT payloads into one stream (side by side on the helper threads), but straight into the pinned
 * buffer, which now holds the COMPRESSED bytes, the palettes and the descriptors; there is one upload; k_png_inflate (one
 * workgroup of one wavefront per zlib stream: csrc/imp_inflate_lanes.h) inflates every stream into its scanline region,
 * which exists only on the device, checks every row's filter byte (and clears one above 4); then the launches of the call without the
 * bit follow unchanged.  *launches is that call's count plus exactly one per group that has a stream to inflate; the groups
 * are the same (IMPGPU_STAGE_CAP_MB counts the device's scanline bytes).  THIS ROUTE WAITS for the device, once per call,
 * for the streams' status words: a stream that is damaged or short, or a filter byte above 4, is IMP_ERROR_DECODE_FAILED
 * with images[i] = NULL, and no other file's result changes.  The calls without the bit still do not wait.  A file whose
 * IDAT payloads exceed 4 GB - 4 KB is IMP_ERROR_UNSUPPORTED on this route.
 * impgpu_image_decode_png_ex with the bit decodes through a batch of one: it does NOT stream rows while inflating (and waits).
 * impgpu_png_info_ex and impgpu_png_scanlines_ex ignore the bit.
 * One wave per stream is slow for one file and pays with many: the measured crossover is in DESIGN.md and README.md. */
#define IMPGPU_PNG_DEVICE_INFLATE 8
/* Diagnostic (host, no device): the wave's own rounds of csrc/imp_inflate_lanes.h, one lane after the other, on one zlib
 * stream in[0, in_size) into exactly out_size bytes of `out`; never reads outside in[], never writes outside out[].
 * IMP_OK, or IMP_ERROR_DECODE_FAILED with *status (may be NULL) the stream's status word: 0 = out_size bytes produced,
 * 1 = damaged, 2 = the input or the final block ended early.  IMP_ERROR_INVALID_ARGS: a NULL buffer, in_size or out_size
 * of 4 GB - 4 KB or more.  The verdict (zero or not) is the host inflate's (impgpu_png_scanlines) on every input but one:
 * a stored block that promises more bytes than the input holds is refused when its header is read, where the host inflate
 * may already have taken up to seven whole bytes its bit buffer held and found the image complete. */
int   impgpu_png_inflate_lanes(const unsigned char* in, size_t in_size, unsigned char* out, size_t out_size, int* status);
int   impgpu_image_wrap(void* device_ptr, int width, int height, int channels, int step,
                        impgpu_image** out);               /* borrow memory already in HBM */
int   impgpu_image_clone(const impgpu_image* src, impgpu_image** out);
int   impgpu_image_download(const impgpu_image* image, unsigned char* data, int step); /* syncs */
/* the same for every frame of an album (bridge.c:680-710 reads them all): all copies are enqueued, then ONE wait */
int   impgpu_batch_download(const impgpu_image* const* images, int count, unsigned char* const* datas, const int* steps);
/* An ALBUM: the frames of one animation (Album, required.h:56-66; filled by LoadGIF, advancedio.c:184-289, or by the
 * one-frame decoders at bridge.c:554-572).  All frames have the canvas' geometry, so they live in ONE device block and
 * the handle stands for all of them: impgpu_run_ops on an album handle runs every operator of the request as ONE launch
 * over all frames (the reference loops `for fid < album.Count` around each operator, bridge.c:577-655), and so does
 * every single operator below.  Info() and ASCII() read frame 0, as bridge.c:283-300 / 669 do; impgpu_image_download*
 * and the batch entry points take single images.  steps may be NULL (= width * channels, tightly packed rows). */
int   impgpu_album_upload(const unsigned char* const* datas, int count, int width, int height, int channels,
                          const int* steps, impgpu_image** out);
int   impgpu_album_download(const impgpu_image* album, unsigned char* const* datas, const int* steps);   /* one wait */
/* impgpu_album_download for `count` handles (0..256; albums and single images mixed) the same way: all copies enqueued,
 * ONE wait.  datas[] / steps[] have one entry per FRAME, handle 0's frames first (sum of impgpu_album_count); steps must
 * be given.  A handle that call refuses gets IMP_ERROR_INVALID_ARGS in codes[i] alone; the fault point it enters
 * (IMP_STEP_ENCODE) is entered per accepted handle, in handle order, before anything is enqueued.  The staging cap cuts
 * the call as it cuts impgpu_batch_download_fi; the return values are that call's too. */
int   impgpu_batch_album_download(const impgpu_image* const* images, int count,
                                  unsigned char* const* datas, const int* steps, int* codes);
int   impgpu_album_count(const impgpu_image* image);        /* 1 for a single image */
int   impgpu_image_width(const impgpu_image* image);
int   impgpu_image_height(const impgpu_image* image);
int   impgpu_image_channels(const impgpu_image* image);
int   impgpu_image_step(const impgpu_image* image);
void* impgpu_image_device_ptr(const impgpu_image* image);
void  impgpu_image_release(impgpu_image** image);          /* cvReleaseImage */

/* ---- operators.  `pointer` operators may replace *pointer and release the old image,
 *      exactly as the reference's IplImage** operators do. ---- */

/* int Crop(IplImage** pointer, char* args, char* gravity)            bridge.h:4, bridge.c:18-141 */
int impgpu_crop(impgpu_image** pointer, const char* args, const char* gravity);
/* int Resize(IplImage** pointer, char* args, Config* config, int simple)  bridge.h:5, bridge.c:143-197 */
int impgpu_resize(impgpu_image** pointer, const char* args, const impgpu_config* config, int simple);
/* cvResize(image, resized, filter)                                    bridge.c:189-191.
 * The reference only ever passes NN / CUBIC (enlarging) / AREA (shrinking); this entry
 * point also takes LINEAR and LANCZOS4 and CUBIC-on-downscale with OpenCV 2.4.9 semantics. */
int impgpu_cv_resize(impgpu_image** pointer, int width, int height, int interpolation);
/* int Filter(IplImage** pointer, char* request, int allowExperiments) filters.h:1, filters.c:43-70 */
int impgpu_filter(impgpu_image** pointer, const char* request, int allow_experiments);
/* int PrepareWatermark(Config* cfg, ngx_pool_t* pool)                 bridge.h:6, bridge.c:199-237.
 * File read + decode stay on the host (cvDecodeImage); this takes the decoded pixels
 * (what bridge.c:221-234 parks in RecoverInfo) and uploads them to HBM. */
int impgpu_prepare_watermark(impgpu_config* config, const unsigned char* pixels, int width,
                             int height, int channels, int step);
/* int Watermark(IplImage* image, Config* config)                      bridge.h:7, bridge.c:239-281 */
int impgpu_watermark(impgpu_image* image, const impgpu_config* config);
/* void BlendWithPaper(IplImage* source)                               filters.h:30, filters.c:666-687 */
int impgpu_blend_with_paper(impgpu_image* image);
/* float CalcPerceivedBrightness(IplImage* image)                      filters.h:34, filters.c:707-729 */
int impgpu_calc_perceived_brightness(const impgpu_image* image, float* brightness);
/* Memory ASCII(IplImage* input, char* args, ngx_pool_t* pool)         filters.h:18, filters.c:486-522.
 * out must hold (width+1)*height-1 bytes; like the reference it leaves the image in HSV. */
int impgpu_ascii(impgpu_image* image, const char* args, unsigned char* out, long capacity, long* length);
/* The two exits above for `count` frames (0..256) at once -- a request queue's json and text answers: launches shared by
 * every frame of a channel count, ONE wait for the device per call.  brightness[i] / codes[i] are what
 * impgpu_calc_perceived_brightness(images[i], &brightness[i]) would give, bit for bit; outs[i] / lengths[i] / codes[i] and
 * the frame's pixels afterwards (HSV) what impgpu_ascii(images[i], args[i], outs[i], capacities[i], &lengths[i]) would.
 * An entry that call would refuse (a NULL handle; for the text a NULL outs[i], fewer than 3 channels, capacities[i] below
 * (width+1)*height-1) gets IMP_ERROR_INVALID_ARGS alone: its frame and buffer are untouched, no other entry changes.
 * args[i] may be NULL (""), and so may args (all "").  An album gives frame 0, as the lone calls do.  The fault point of
 * the brightness call (IMP_STEP_INFO) is entered per non-NULL entry, in entry order, before anything is launched; an
 * entry whose point fires gets IMP_ERROR_DEVICE and is left out, the rest is served.  A shared launch that fails gives
 * every entry in it IMP_ERROR_DEVICE.  launches (may be NULL) receives the number of kernels enqueued: at most two per
 * channel count present for the brightness (one when no frame of it has 4113 pixels), one per channel count for the
 * text, whatever `count` is.  IMP_ERROR_INVALID_ARGS with nothing enqueued for NULL arrays (count > 0), a count outside
 * 0..256 and -- impgpu_batch_ascii writes its frames in place -- the same handle twice (the brightness only reads:
 * repeats are allowed there); IMP_ERROR_DEVICE without an env (every codes[i] says so too); otherwise IMP_OK, and the
 * verdicts are in codes[].  Both return with their answers: the wait is inside. */
int impgpu_batch_calc_perceived_brightness(const impgpu_image* const* images, int count, float* brightness, int* codes,
                                           int* launches);
int impgpu_batch_ascii(impgpu_image* const* images, const char* const* args, int count, unsigned char* const* outs,
                       const long* capacities, long* lengths, int* codes, int* launches);
/* cvCvtColor(image, colored, CV_GRAY2BGR)                             bridge.c:613-618 */
int impgpu_gray2bgr(impgpu_image** pointer);
/* void RGB2HSV(IplImage*) / void HSV2RGB(IplImage*)                   helpers.h:17-18, helpers.c:70-176 */
int impgpu_rgb2hsv(impgpu_image* image);
int impgpu_hsv2rgb(impgpu_image* image);

/* The operator segment of RunJob, bridge.c:574-656: crop -> resize -> [gray->BGR] ->
 * filters in order -> watermark -> flatten.  *step receives the IMP_STEP_* that was
 * running when a non-zero code was returned (JobResult.Step, required.h:78-84).
 * Crop is folded into the next operator's source view, consecutive pointwise filters
 * run as one kernel. */
int impgpu_run_ops(impgpu_image** pointer, const impgpu_job* job, const impgpu_config* config, int* step);
/* The operator segment of RunJob (impgpu_run_ops) for `count` independent requests at once -- a request queue's worth, each
 * with its own job and config.  On return images[i], codes[i] and steps[i] are exactly what
 * impgpu_run_ops(&images[i], &jobs[i], configs[i], &steps[i]) would have left, in request order; the fault points
 * (impgpu_fault_arm) are entered in the same order as by that loop, before anything is launched.  A single BGR / BGRA
 * frame whose chain is [crop ->] resize (general INTER_AREA) [-> one filter-rotate] [-> a BGRA overlay] [-> flatten] rides
 * ONE launch per channel count with every other such request, the tail on the resize's stores (bare resizes share the
 * launch of impgpu_batch_resize_mixed).  Any other single BGR / BGRA frame whose chain is [crop ->] resize -> any filters
 * -> [watermark] -> [flatten] shares launches in rounds: the resizes first, then round k launches the k-th segment of every
 * chain that has one -- a run of pointwise filters (with the watermark and the flatten when it is the last), a blur, or a
 * flip / turn -- one launch per kind and channel count, so the number of launches follows the chains' length, not the
 * number of requests.  Bare resizes with whole factors (resizeAreaFast_: 1280x720 or 1920x1080 at 320 wide) share one
 * launch per channel count too, and so do the NN resizes of `simple` requests and the BGR / BGRA enlargements (CUBIC) -- at
 * most five resize launches per channel count.  Resizes launch_resize_mixed does not gather (gray enlargements, frames of
 * which one axis grows while y shrinks, enlargements whose x shrinks past 2x, extreme ratios: cells past 66 source
 * columns) still take a launch per request inside their round.  Blurs share launches by form: the one-pass forms (small
 * radii) one launch per form and byte-plane count, the two-pass matrix-unit form (impgpu_blur_form 3: from sigma 5.6 / 6.6
 * for BGRA / BGR up, through sigma 25 and beyond while the trimmed radius stays within 56; blur=8 among them) ONE launch pair and one planes buffer per channel count and plane count -- unless the
 * round holds a single such frame, which runs alone as in impgpu_run_ops; the remaining forms (impgpu_blur_form 0: radii past
 * 56, tap sums no matrix-unit form takes, 1-pixel axes, BGRA windows off the dword grid) take their launches per request.
 * A single GRAY frame with a resize rides the same launches: its resize joins the gray
 * group of impgpu_batch_resize_mixed (channels = 1), ONE k_gray2bgr_mix launch then promotes every gray request of the call
 * (bridge.c:613-618, the filtering step -- entered for a gray frame even without filters; a request whose fault point fires
 * there keeps its resized gray frame), and from there its chain's segments run in the 3-channel groups with the call's BGR
 * requests: no turn rides a gray resize, the overlay (3 or 4 channels) is always the tail's, there is never a flatten.  A
 * call of gray bare resizes is at most three resize launches plus the promotion.  A single frame WITHOUT a resize -- a
 * crop alone, a watermark-only location, filters on an original -- shares launches too: its chain [crop ->] any filters ->
 * [watermark] -> [flatten] is the same list of segments, and its first segment reads the crop window.  A gray one is
 * promoted from its window by the call's single promotion launch (shared with the resized gray requests).  A colour one
 * whose first segment is pointwise (or the watermark / flatten tail) leaves its window through ONE window launch per
 * channel count -- two when some programs have a vignette stage -- that reads the window, runs that segment and writes the
 * fresh frame; the bare crop is an item of the same launch whose rows move as 16-byte runs; a flip, turn or one-pass blur
 * takes the window as its source in its round's launch.  Later segments run in the rounds above.  When the window is the
 * whole frame everything runs in place and the handle stays, as impgpu_run_ops leaves it; with no segment at all nothing is
 * launched.  For its requests without a resize a call therefore makes at most one promotion, two window launches per colour
 * channel count and what their later rounds cost, whatever `count` is (a request that still stands on its window after a
 * blur that worked in place is copied out by one more window launch behind its last round).  A request cut by a fault
 * point keeps what impgpu_run_ops leaves: its uncropped frame, with the pointwise filters applied inside the window when
 * the watermark step was the one that fired.  A BGR / BGRA ALBUM (GIF composes and FreeImage frames are BGRA) rides the same
 * launches: it is planned once per request -- crop, resize geometry, filter plans and overlay placement are the same for all
 * its frames -- and every frame is an item of its own in each launch its request takes part in, so N albums cost the
 * launches their frames would cost as single images, not N times the chain's length.  The handle stays ONE album in one block
 * with the same frame count, as impgpu_run_ops leaves it; its fault points are entered once per request and step, never per
 * frame; a blur form that runs alone, and a two-pass blur that is the only REQUEST of its class in its round, is one launch
 * (pair) over all frames of the album, as in impgpu_run_ops.  A call takes at most 4096 album frames into its shared launches:
 * the albums past that bound, in request order, go through impgpu_run_ops inside the call, and so does every GRAY album
 * (1 channel), and an album that is the only colour album of its call (its operators are one launch each over all its
 * frames there already).  Requests whose arguments fail (a bad crop, an unknown filter, too
 * many filters, a watermark that does not fit) go through impgpu_run_ops inside the call too.  A shared launch that fails gives
 * each of its requests IMP_ERROR_DEVICE with the step of the segment it ran, and each keeps the frame it had.  launches (may be NULL) receives the number of kernels enqueued.  IMP_ERROR_INVALID_ARGS
 * with nothing enqueued when the arguments are malformed (NULL arrays, count < 0 or > 4096, the same handle twice); IMP_ERROR_DEVICE without an env (every codes[i] says so too);
 * otherwise IMP_OK, and the verdicts are in codes[].  Asynchronous on the env stream, like impgpu_run_ops. */
int impgpu_batch_run_ops(impgpu_image** images, const impgpu_job* jobs, const impgpu_config* const* configs,
                         int count, int* codes, int* steps, int* launches);

/* ---- argument grammar only (host, no device): what Crop / Resize decide before they
 *      touch pixels.  Used by the module to answer 400/405/413 without a GPU round trip. ---- */
int impgpu_crop_geometry(int width, int height, const char* args, const char* gravity,
                         int* x, int* y, int* w, int* h);                      /* bridge.c:18-128 */
int impgpu_resize_geometry(int width, int height, const char* args, const impgpu_config* config,
                           int simple, int* w, int* h, int* interpolation);   /* bridge.c:143-190 */
int impgpu_filter_check(const char* request, int allow_experiments);           /* filters.c:43-70 + per-filter arg checks */
int impgpu_check_destructive(const char* request);                             /* filters.c:32-40 */
/* Which Gaussian form a dword-aligned width x height frame of 3 or 4 channels gets for filter-blur=sigma (host, no device):
 * 1 = k_blur_fused4, 2 = the one-pass matrix-unit form, 3 = the two-pass matrix-unit form (rows, planes buffer, columns) --
 * the forms whose frames share launches in impgpu_batch_run_ops -- 0 = any other form (other channel counts and 1-pixel axes
 * included).  *planes (may be NULL) = the byte planes of the row sums for forms 2 and 3 (2, or 3 when the fixed-point taps sum
 * to 258..260), else 0: frames share a launch only with frames of the same form and plane count. */
int impgpu_blur_form(int width, int height, int channels, double sigma, int* planes);

/* ---- request front end (host, no device): the part of RunJob above the operators.
 *      URI unescape + GET grammar of bridge.c:304-372 ('?' split, '&' tokens, prefix-matched keys,
 *      last crop/gravity/resize/quality/format/page wins, filters appended up to
 *      config->max_filters_count) and the encoder choice of bridge.c:413-466 that decides
 *      job.simple (GIF, bridge.c:594) and job.need_flatten (bridge.c:642-648).
 *      `extension` is req->exten, used when format= is absent (bridge.c:413-416).
 *      On error *out is still a valid object to free. The job's strings live inside it. ---- */
typedef struct impgpu_request impgpu_request;
int               impgpu_parse_request(const char* uri, const char* extension, const impgpu_config* config,
                                       impgpu_request** out);
const impgpu_job* impgpu_request_job(const impgpu_request* request);
const char*       impgpu_request_quality(const impgpu_request* request);    /* value of quality= or NULL */
const char*       impgpu_request_format(const impgpu_request* request);     /* value of format= or NULL */
/* the page LoadGIF gets (DecodeRequest.Page, bridge.c:563): the page= value; when absent, 0 for every encoder that
 * takes one frame and -1 (= all pages) only for GIF output and the json exit (bridge.c:324, :433-435, :448-450) */
int               impgpu_request_page(const impgpu_request* request);
int               impgpu_request_mime(const impgpu_request* request);       /* IMP_MIME_* of required.h:57-62 */
int               impgpu_request_destructive(const impgpu_request* request); /* CheckDestructive over the filters */
void              impgpu_request_free(impgpu_request** request);

/* ---- GIF album hand-over: LoadGIF (advancedio.c:103-262).  Here FreeImage decodes the pages on the host (the calls
 *      that take the FILE follow below); the
 *      per-pixel compositing loop of advancedio.c:204-247 -- the frame placed at FrameLeft/FrameTop on the first
 *      page's canvas, the transparent index, the `master` index canvas carried from page to page when the request
 *      is destructive (advancedio.c:195-240), the RGBQUAD palette lookup into a 4-channel frame (:242-246) -- runs
 *      on the device.  A page is what FreeImage hands that loop: 8-bit indices in scanline order (bottom-up,
 *      `pitch` bytes per row; FreeImage_ConvertTo8Bits first when the page is not 8-bit, :181-185).
 *      frames[i] = page i (all `count` of them) when page == -1.  With page >= 0 the walk is always destructive, a
 *      page past the last one means page 0 (advancedio.c:111-116), the walk stops at that page and frames[0] is
 *      that page alone (advancedio.c:256-273).  page < -1 returns IMP_ERROR_INVALID_ARGS (undefined in the reference). ---- */
#define IMP_GIF_DISPOSAL_UNSPECIFIED 0
#define IMP_GIF_DISPOSAL_LEAVE       1
#define IMP_GIF_DISPOSAL_BACKGROUND  2
#define IMP_GIF_DISPOSAL_PREVIOUS    3
typedef struct impgpu_gif_page {
    const unsigned char* indices;   /* FreeImage_GetBits of the 8-bit page (host memory) */
    int width, height, pitch;       /* FreeImage_GetWidth / GetHeight / GetPitch */
    int left, top;                  /* FIMD_ANIMATION FrameLeft / FrameTop (advancedio.c:159-174) */
    int dispose;                    /* FIMD_ANIMATION DisposalMethod (advancedio.c:146-157) -> Frame.Dispose */
    int transparency_key;           /* FreeImage_GetTransparentIndex, -1 = none (advancedio.c:176) */
    const unsigned char* palette;   /* FreeImage_GetPalette: 256 RGBQUAD = B,G,R,reserved bytes (advancedio.c:178) */
} impgpu_gif_page;
int impgpu_gif_compose(const impgpu_gif_page* pages, int count, int destructive, int page, impgpu_image** frames);
/* the same frames as ONE album handle (see impgpu_album_upload): what RunJob's operator segment then runs on */
int impgpu_gif_compose_album(const impgpu_gif_page* pages, int count, int destructive, int page, impgpu_image** album);
/* MANY files, ONE compose launch (what the broker does with the GIF uploads of a batch).  albums[i] / codes[i] are exactly
 * what impgpu_gif_compose_album(sets[i].pages, sets[i].count, sets[i].destructive, sets[i].page, &albums[i]) gives alone,
 * pixel for pixel; an entry that call refuses gets its code alone (albums[i] = NULL) and changes no other entry.  All
 * accepted entries' page tables, palettes and indices travel in one staging blob -- one upload, built in pinned memory and
 * sent in pieces while the rest is still being copied in -- and one launch
 * (k_gif_compose_mix, a descriptor per album) composes them: *launches (may be NULL) is 1 when any entry was accepted and
 * 0 otherwise.  Only a blob that would pass $IMPGPU_STAGE_CAP_MB is cut, at an entry: one upload and launch per group, in
 * entry order.  count is 0..256; NULL arrays with count > 0 or a count outside the range return IMP_ERROR_INVALID_ARGS
 * with nothing enqueued; without an env the call returns IMP_ERROR_DEVICE and so does every codes[i].  Asynchronous like
 * the lone call: the page memory is read before it returns. */
typedef struct impgpu_gif_set { const impgpu_gif_page* pages; int count, destructive, page; } impgpu_gif_set;
int impgpu_batch_gif_compose(const impgpu_gif_set* sets, int count, impgpu_image** albums, int* codes, int* launches);

/* ---- GIF FILES in: the hand-over above still has FreeImage LZW-decode every page on a host core and ship index planes
 *      of 2-5x the file's size.  These calls take the file.  The host walks the container (include/impgpu_gif.h:
 *      impgpu_gif_walk, which decompresses nothing); the compressed sub-block payloads are uploaded, k_gif_lzw decodes
 *      every page -- one wavefront per page, the table in LDS, rounds of 64 codes whose bit offsets are a closed form of
 *      the round's start state -- straight into the index planes the compositing loop reads (8-bit, bottom-up, pitch =
 *      (width + 3) & ~3, pad bytes 0: what FreeImage would hold), and k_gif_compose_mix follows on the same stream.
 *      *album is what impgpu_gif_compose_album gives for the file's pages (`destructive` and `page` as there; pages
 *      behind a requested page are neither decoded nor judged; page < -1: IMP_ERROR_INVALID_ARGS).
 *      TAKEN: GIF87a / GIF89a, local and global colour tables of 2..256 entries, min_code_size 2..8, interlaced pages,
 *      clear codes anywhere including none after the table filled (deferred clear), sides up to 4096, up to 4096 pages.
 *      REFUSED, IMP_ERROR_UNSUPPORTED (the host decoder's): another signature, a page with no colour table,
 *      min_code_size outside 2..8, a side above 4096, more than 4096 pages, no page, index planes past 1 GB, a page of
 *      256 MB or more compressed.
 *      IMP_ERROR_DECODE_FAILED: a block or sub-block chain past the file's end, a page of zero size, an unknown block
 *      introducer, no trailer -- and, by the DEVICE's verdict (a status word per page), a code above the next free code, a
 *      first code after a clear that is not a literal, data that ends before width x height indices, indices beyond them.
 *      A damaged stream never writes outside its page's plane.  The call waits ONCE, for the status words; no album is
 *      returned for a damaged file.  The canvas is page 0's size (advancedio.c:134-137), not the logical screen.
 *      MEASURED (profiles/gif_decode_probe.json; the host side is the library's own plain decoder on
 *      one thread, impgpu_gif_pages(how = 0), NOT FreeImage, which is not installed): one wave per page is slow for one
 *      page -- a lone 640x480 page 8.3 ms against 1.0 ms, 320x240 1.9 against 0.26 -- level with the host at about 8
 *      pages in the call, ahead beyond: a 64-page 640x480 file 9.7 against 63 ms, 64 albums of 8 pages at 320x240 3.0
 *      against 121 ms.  Not measured: FreeImage's decoder, many host workers decoding side by side, the broker (which
 *      does not call this path; it has no option for it yet). ---- */
int impgpu_image_decode_gif(const unsigned char* blob, size_t size, int destructive, int page, impgpu_image** album);
/* MANY files: one upload, ONE k_gif_lzw launch and ONE k_gif_compose_mix launch for the whole call -- *launches (may be
 * NULL) is 2, or 0 when no file was accepted.  codes[i] / albums[i] are exactly the lone call's; a refused or damaged
 * file gets its code alone and changes no other file.  Cut at a file only by $IMPGPU_STAGE_CAP_MB (two launches per
 * group, in file order).  count is 0..256; NULL arrays with count > 0 or a count outside the range return
 * IMP_ERROR_INVALID_ARGS with nothing enqueued; without an env the call returns IMP_ERROR_DEVICE and so does every codes[i]. */
int impgpu_batch_decode_gif(const unsigned char* const* blobs, const size_t* sizes, const int* destructive, const int* page,
                            int count, impgpu_image** albums, int* codes, int* launches);
/* host only: the page count and the canvas (page 0's size) of a file these calls would take; impgpu_gif_walk's verdict */
int impgpu_gif_info(const unsigned char* blob, size_t size, int* count, int* canvas_width, int* canvas_height);
/* host only, a diagnostic: the index planes of every page in the layout above, one after the other, into `out`
 * (*length = their bytes; IMP_ERROR_MALLOC_FAILED when `capacity` is less, or `out` is NULL).  how = 0: a plain
 * sequential LZW decoder; how = 1: the wave's rounds (csrc/imp_gif.h, the kernel's own lane code) one lane after the
 * other.  A damaged page makes the call IMP_ERROR_DECODE_FAILED; nothing outside the planes is written. */
int impgpu_gif_pages(const unsigned char* blob, size_t size, int how, unsigned char* out, size_t capacity, size_t* length);
/* ---- the same calls with `flags`.  flags == 0 is the call above in every respect: answers, codes, *launches == 2.  Any bit
 *      other than IMPGPU_GIF_SPLIT is IMP_ERROR_INVALID_ARGS before a device is looked for.
 *      IMPGPU_GIF_SPLIT (opt-in; the route never switches by size on its own): LZW is sequential only BETWEEN clear codes --
 *      behind one the decoder's state is known (an empty table, codes of min_code_size + 1 bits), and every mainstream
 *      encoder clears when the table fills, every 5.4 KB of noise at min_code_size 8.  So a page is cut at its clear
 *      codes and a wavefront decodes every SEGMENT.  Four launches per group where the call above makes two:
 *        k_gif_lzw_scan  a wavefront per page walks the codes WITHOUT a table (a code's width depends only on the count
 *                        of codes since the last clear; rounds of 1024 codes, 16 per lane, their loads in flight
 *                        together) and writes the page's segments {start bit, end bit}.  Segment 0
 *                        starts at bit 0.  THE CUT RULE: a clear code is a cut -- the segment ends just behind it and
 *                        the next starts there -- when at least IMPGPU_GIF_SPLIT_MIN_BYTES of stream lie between the
 *                        segment's start and the bit behind the clear (and the page's table of data_bytes /
 *                        IMPGPU_GIF_SPLIT_MIN_BYTES + 1 segments has room, which it always has); any other clear stays
 *                        inside its segment and is handled by that segment's decoder like in the one-wave route.  The
 *                        scan stops where a decoder would stop for a reason visible without a table: end-of-information,
 *                        no data, a code above the free code, a first-after-clear code that is no literal.
 *        k_gif_lzw_len   a wavefront per segment SLOT (the grid is the host's bound, the sum of the pages' table sizes;
 *                        a slot at or past the page's count returns at once): the rounds without their stores -- how
 *                        many indices the segment holds, and whether it ended on an invalid code.
 *        k_gif_lzw_emit  a wavefront per slot: the same rounds with their stores, at the sum of the earlier segments'
 *                        lengths; segment 0's wavefront writes the pad bytes and the page's status word, folded from
 *                        the segments' records in stream order to exactly the one-wave decoder's verdict.  (A page of
 *                        ONE segment skips the length pass: its emit wavefront runs the one-wave loop.)
 *        k_gif_compose_mix  as above.
 *      Every stage reads what the stage before wrote across a kernel boundary of one stream: no wavefront waits for
 *      another workgroup.  Upload, plane layout, grouping by $IMPGPU_STAGE_CAP_MB, the status word per page, the one
 *      wait, refusals, codes and albums are the flag-less call's, file by file; the segment tables lie in the same
 *      device block behind the planes.  Which clears become cuts changes no answer.
 *      MEASURED (profiles/gif_split_probe.json, one session, the one-wave route and the library's plain
 *      host decoder on one thread beside it; ms per call): a lone 640x480 page of 33 segments 1.09 against 6.43 one-wave and
 *      0.65 host; a photo-like 640x480 page of 52 segments 1.48 / 9.87 / 1.18; a 1920x1080 page of 407 segments 9.0 / 77.3 /
 *      8.7; an 8-page 640x480 file 1.20 / 6.62 / 5.28; 64 single-page 640x480 files 1.97 / 6.90 / 41.2.  The split route
 *      is 2-8.5x the one-wave route wherever a page has several segments and a call has fewer segments than the device
 *      runs side by side; it is level (within 10 %) for single-segment pages and for calls of 512 pages, and
 *      BEHIND at 64 albums of 64 pages at 320x240 (18.3 against 15.9 ms: the rounds run twice).  A LONE page is still
 *      behind one host core (1.7x at 640x480, level at 1080p): k_gif_lzw_scan, the one sequential walk that is left, takes
 *      0.67 of the 1.09 ms (len 0.16, emit 0.20).  IMPGPU_GIF_SPLIT_MIN_BYTES has not been tuned. ---- */
#define IMPGPU_GIF_SPLIT 1
#define IMPGPU_GIF_SPLIT_MIN_BYTES 2048
int impgpu_image_decode_gif_ex(const unsigned char* blob, size_t size, int destructive, int page, int flags, impgpu_image** album);
/* *launches (may be NULL): 4 per group with IMPGPU_GIF_SPLIT, 2 without, 0 when no file was accepted */
int impgpu_batch_decode_gif_ex(const unsigned char* const* blobs, const size_t* sizes, const int* destructive, const int* page,
                               int count, int flags, impgpu_image** albums, int* codes, int* launches);
/* host, no device: the planes as impgpu_gif_pages lays them out, made by the three passes' own lane code run one lane after
 * the other; segments[f] (may be NULL; pages_capacity entries) = the number of segments page f was cut into */
int impgpu_gif_pages_split(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, size_t* length,
                           int* segments, int pages_capacity);

/* ---- GIF FILES out: SaveGIF (advancedio.c:340-425) has a host core quantise and LZW-encode every page of the 32-bit
 *      frames impgpu_batch_album_download ships.  These calls write the FILE on the device.  The reference's GIF resize is
 *      nearest-neighbour, and crop, flips, turns and every pointwise filter give a frame no colour its source page did not
 *      have: for those requests the palette is EXACT and nothing is quantised.  The file is not FreeImage's bytes (its
 *      NNQUANT palette cannot be pinned where FreeImage is not installed) but defined here, deterministically:
 *      a pixel is TRANSPARENT when its frame has 4 channels and its alpha byte is 0 (any other alpha is ignored); a frame's
 *      colour set is the distinct (R,G,B) of its other pixels.  With U the union of the sets and T = some frame has a
 *      transparent pixel: |U| + T <= 256 gives ONE global table and no local ones; otherwise no global table and a local
 *      table per frame, of its own set.  A table lists its colours ascending by R<<16 | G<<8 | B, then the transparent entry
 *      (stored 0,0,0) when it has one, padded with 0,0,0 to a power of two >= 2; min_code_size = max(2, log2(size)).
 *      Indices in top-down raster order, no interlace.  LZW: greedy, 12 bits, a clear code at the start, in front of pixel
 *      k * segment (the pending code first) and whenever the table is full and another entry is due; widths as the decoder
 *      sees them; end-of-information.  Container: GIF89a, the w x h screen, flags 0xF0 | bits with a global table and 0x70
 *      without, NETSCAPE2.0 when loop_count >= 0, per frame a graphic control extension (dispose[i], the transparency flag
 *      and index iff the frame has a transparent pixel, delay min(65535, time_ms[i] / 10)), the image descriptor at 0,0,
 *      255-byte sub-blocks; the trailer.  tests/gif_writer.py writes the same bytes.
 *      time_ms / dispose: Frame.Time / Frame.Dispose (required.h:129-140; the handle does not carry them), NULL = all 0.
 *      A single image is an album of one.  segment = 0 means IMPGPU_GIF_ENC_SEGMENT.
 *      TAKEN: 3- and 4-channel frames up to 4096 x 4096, up to 4096 frames (what impgpu_image_decode_gif takes back).
 *      REFUSED, IMP_ERROR_INVALID_ARGS before a device is looked for: a segment outside {0} and [256, 2^24], a dispose
 *      outside 0..3, loop_count > 65535.  IMP_ERROR_UNSUPPORTED, *length = 0, nothing written: 1- or 2-channel frames, a
 *      larger side, more frames, a frame whose colours (and transparency) fit no table of 256 -- blur, vignette or a
 *      watermark do that: use the _ex calls with IMPGPU_GIF_ENC_QUANTIZE (below), or download the frames and quantise on
 *      the host as before.  IMP_ERROR_MALLOC_FAILED: `capacity`
 *      is too small; nothing is written, *length is the size needed; impgpu_gif_encode_bound is always enough.
 *      FIVE launches for a call, whatever it holds: k_gif_enc_sets (a colour set per frame: an LDS hash set per workgroup,
 *      then compare-and-swap into the frame's), k_gif_enc_tables (a workgroup per album sorts the sets, unites them and
 *      decides), k_gif_enc_index (table in LDS, a bisection per pixel), k_gif_enc_lzw (a wavefront per SEGMENT: the greedy
 *      walk is sequential and wave-uniform over an LDS hash table, 64 lanes pack 64 codes at a time) and k_gif_enc_pack
 *      (prefix sum of the segments' bit lengths, whole bytes into 255-byte sub-blocks).  TWO waits: the frames' records
 *      (verdict, table size, stream length), then the tables and streams of the files that fit.
 *      MEASURED (profiles/gif_encode_probe.json, one session, dithered 256-colour frames; the host side
 *      is impgpu_gif_encode_host on one thread, NOT FreeImage, which is not installed): a lone 640x480 frame 2.01 ms, 8
 *      frames 2.29 ms, 64 albums of 8 frames at 320x240 21.2 ms -- against 0.08 / 0.51 / 11.3 ms for impgpu_batch_album_download
 *      of the 32-bit frames alone and 7.0 / 56.8 / 818 ms for that plus the host encoder: 3.5x / 25x / 39x the host route,
 *      4.3-4.8x fewer bytes across the link, but BEHIND the bare download.  Correct, not fast: k_gif_enc_lzw is 1.90 of the
 *      2.29 ms (a segment's walk costs about 230 ns a pixel); the other four launches together 0.11 ms.  The cut at 8192
 *      costs x0.99 (noise), x1.02 (dither), x1.5 (flat colour) in file size; 3584 and 32768 were measured too. ---- */
#define IMPGPU_GIF_ENC_SEGMENT 8192
int impgpu_album_encode_gif(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment,
                            unsigned char* out, size_t capacity, size_t* length);
/* MANY albums (count 0..256): codes[i] / lengths[i] / the file are exactly the lone call's; a refused album gets its code
 * alone and changes no other entry.  time_ms / dispose may be NULL, and so may their entries.  *launches (may be NULL): the
 * kernels enqueued -- 5 for a call under $IMPGPU_STAGE_CAP_MB (measured by impgpu_gif_encode_bound), whatever count and the
 * frame counts are; 0 when no album was accepted.  IMP_ERROR_INVALID_ARGS for NULL arrays with count > 0, a count outside
 * 0..256 or a bad segment; IMP_ERROR_DEVICE without an env (every codes[i] says so too). */
int impgpu_batch_encode_gif(const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                            const int* loop_counts, int count, int segment, unsigned char* const* outs,
                            const size_t* capacities, size_t* lengths, int* codes, int* launches);
/* a size no file of `frames` frames of width x height exceeds (0: a geometry the calls refuse) */
size_t impgpu_gif_encode_bound(int width, int height, int frames);
/* host, no device: the same file from frames in host memory (B,G,R[,A] rows `step` bytes apart), made by the launches'
 * own lane code (csrc/imp_gif_enc.h) run one lane after the other on one thread */
int impgpu_gif_encode_host(const unsigned char* const* frames, int count, int width, int height, int channels, int step,
                           const int* time_ms, const int* dispose, int loop_count, int segment,
                           unsigned char* out, size_t capacity, size_t* length);

/* ---- GIF FILES out, PAST 256 COLOURS (opt-in): the calls above with a `flags` argument.  flags = 0 IS the call without
 *      _ex in every respect -- files, codes, refusals, launches, waits -- and the calls without _ex keep refusing.  A flag
 *      bit other than IMPGPU_GIF_ENC_QUANTIZE: IMP_ERROR_INVALID_ARGS before a device is looked for.
 *      IMPGPU_GIF_ENC_QUANTIZE extends the file's definition above to a frame whose OWN key set (its colours, plus
 *      "transparent") exceeds 256 -- a watermark, a blur, a vignette, an overlay, a non-NN resize do that.  An album with
 *      such a frame has no global table; its other frames keep the exact local tables of their own sets; such a frame's
 *      local table and indices are, all in integers, with no dithering and no nearest-colour search:
 *      1. KEYS.  T = 1 if the frame has a transparent pixel, else 0; K = 256 - T.  Transparent pixels take no part in 2-5.
 *      2. HISTOGRAM.  A pixel's cell is (R>>3, G>>3, B>>3).  Each of the 32768 cells holds four unsigned 32-bit sums over
 *         its pixels: the count n and the sums of R, G and B (full 8-bit values).  4096 x 4096 pixels keep them below 2^32.
 *      3. BOXES.  A box is an inclusive cell range on each axis, always shrunk to the tight bounds of its non-empty cells.
 *         Start with one box around all non-empty cells.  While there are fewer than K boxes: among the boxes whose longest
 *         side s = max(r1-r0, g1-g0, b1-b0) is > 0 take the one with the largest n * s (ties: the lowest box number; none:
 *         stop) and cut it across its longest axis (ties: R, then G, then B).  With m[j] the box's pixels in plane j of
 *         that axis (j = 0..s), t = the smallest j with m[0] + ... + m[j] >= ceil(n / 2), at most s - 1.  Planes 0..t keep
 *         the box's number, planes t+1..s become box number (current box count); both are shrunk to tight bounds.
 *      4. COLOURS.  A box's colour per channel is (2 * sum + n) / (2 * n) in integer division, from the box's sums.  Boxes
 *         are disjoint and a mean lies inside its box, so the colours are distinct.
 *      5. TABLE AND INDICES.  The table lists the box colours ascending by R<<16 | G<<8 | B, then the transparent entry
 *         when T; padding, min_code_size and the rest as above; nkeys = boxes + T.  A pixel's index is the rank of the box
 *         its cell lies in; a transparent pixel's is nkeys - 1.
 *      The sums do not depend on the order of the additions: the device's atomics give the same file on every run.  An
 *      album whose frames all fit gets exactly the file it gets without the flag.
 *      EIGHT launches for a group of albums under the flag, whatever it holds: k_gif_enc_sets, k_gif_enc_claim (one
 *      workgroup hands the pool's histogram slots to the frames that overflowed, a whole album or none of it),
 *      k_gif_enc_hist (the 4096-pixel items again; equal cells are combined in a lane's registers and in an LDS table
 *      before they reach device memory), k_gif_enc_cut (a workgroup per slot: a summed-volume table of the counts in 128 KB
 *      of LDS, up to 255 cuts, the table, the record and a 32768-byte cell -> index table), k_gif_enc_tables,
 *      k_gif_enc_index (a quantised frame's pixels go through the cell -> index table, staged in LDS), k_gif_enc_lzw and
 *      k_gif_enc_pack.  A slot is 544 KB; the pool holds as many as fit under $IMPGPU_STAGE_CAP_MB (at least one, at most
 *      one per frame of the group).  An album that got no slots is encoded by the same call in a FURTHER group of eight
 *      launches, whose pool holds what its albums need; *launches is 8 x the groups.  Two waits per group.
 *      impgpu_gif_encode_bound holds unchanged: the stream's bound does not depend on the table.
 *      MEASURED (profiles/gif_quant_probe.json, one session, photo frames of 189 k colours): a lone
 *      640x480 frame 2.75 ms, 8 frames 3.08 ms, 64 albums of 8 frames at 320x240 25.2 ms -- against 0.10 / 0.67 / 12.7 ms for
 *      the frames' download alone and 7.7 / 61.5 / 1386 ms for that plus impgpu_gif_encode_host_ex on one thread.  Per launch
 *      for the 8 frames: k_gif_enc_lzw 1735 us, k_gif_enc_cut 931, k_gif_enc_hist 106, the other five 46 together. ---- */
#define IMPGPU_GIF_ENC_QUANTIZE 1
int impgpu_album_encode_gif_ex(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment,
                               int flags, unsigned char* out, size_t capacity, size_t* length);
int impgpu_batch_encode_gif_ex(const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                               const int* loop_counts, int count, int segment, int flags, unsigned char* const* outs,
                               const size_t* capacities, size_t* lengths, int* codes, int* launches);
int impgpu_gif_encode_host_ex(const unsigned char* const* frames, int count, int width, int height, int channels, int step,
                              const int* time_ms, const int* dispose, int loop_count, int segment, int flags,
                              unsigned char* out, size_t capacity, size_t* length);
/* diagnostic, host, no device: steps 1-5 on ONE frame, whatever its colour count: table = *entries x (R,G,B) bytes (room
 * for 768; the transparent entry is 0,0,0), *entries = nkeys, *transparent_index = nkeys - 1 or -1, indices = width x height
 * bytes in raster order.  Geometry and step are checked as by impgpu_gif_encode_host. */
int impgpu_gif_quantize_host(const unsigned char* frame, int width, int height, int channels, int step,
                             unsigned char* table, int* entries, int* transparent_index, unsigned char* indices);

/* ---- GIF FILES out, DELTA FRAMES (opt-in): the _ex calls again, as _ex2, whose `flags` may hold IMPGPU_GIF_ENC_QUANTIZE |
 *      IMPGPU_GIF_ENC_DELTA.  Any other bit: IMP_ERROR_INVALID_ARGS before a device is looked for.  Without the DELTA bit an
 *      _ex2 call IS the _ex call -- files, codes, refusals, launches and waits -- and the _ex calls keep refusing the bit.
 *      Why: a request with a destructive filter (blur, vignette) or a page extraction restores every frame to a full canvas
 *      (advancedio.c:195-240), and the answer loses GIF's inter-frame compression.  Under the bit a pixel equal to the pixel
 *      under it in the previous frame is written as transparent, and the frame shrinks to the rectangle that changed.
 *      THE FILE.  Everything in the definitions above stands.  Under IMPGPU_GIF_ENC_DELTA, with d(i) = dispose[i] (0 where
 *      dispose is NULL):
 *      1. DELTA FRAMES.  Frame i is a CANDIDATE iff i >= 1, d(i-1) is 0 or 1, and d(i) is 0 or 1.  Frame 0 is never a
 *         candidate.  A frame behind a "restore to background / previous" is never a candidate.  A frame that itself asks
 *         for one is never a candidate either, because its disposal area would shrink with its window.
 *      2. HELD PIXELS.  In a candidate, pixel p is HELD iff its key is a colour and equals the key of pixel p of frame i-1.
 *         Keys are as defined today: GIF_KEY_TRANSPARENT for alpha 0 of a 4-channel frame, else the R,G,B.  The keys are
 *         those of the caller's frames.  They are never a quantised colour and never what was written for frame i-1.  A
 *         transparent pixel is never held.
 *      3. WINDOW.  The window is the smallest rectangle x0,y0,ww,wh that contains every pixel that is not held.  If every
 *         pixel is held, the window is the 1 x 1 rectangle at 0,0.  Outside the window every pixel is held.
 *      4. WRITTEN KEYS.  In window raster order, a held pixel is written as GIF_KEY_TRANSPARENT and any other pixel keeps
 *         its own key.  Set A is the set of written keys.  Set B is the frame's own key set over the whole frame, which is
 *         today's set.
 *      5. CHOICE, per candidate.  |A| <= 256: the frame is a DELTA FRAME.  Its "frame" for every later rule (union and
 *         global-table decision, table, has_trans, indices, LZW, segments, which count window pixels) is the written window
 *         with set A.  Else |B| <= 256: the frame is written PLAIN, exactly as without the bit.  Else, with
 *         IMPGPU_GIF_ENC_QUANTIZE: the frame is a delta frame and is quantised.  Steps 1-5 of the quantiser run over the
 *         window's pixels that are neither held nor transparent.  T = 1 iff the window has a held or a transparent pixel.
 *         A held pixel's index is nkeys - 1.  Else: the album is refused as today.  A non-candidate frame is written as
 *         without the bit.  So the bit never refuses an album the call without it takes, and it never quantises a frame the
 *         call without it writes exactly.
 *      6. CONTAINER.  A delta frame's image descriptor is x0, y0, ww, wh.  Its graphic control extension carries the
 *         caller's dispose[i] and delay unchanged.  The transparency flag and index follow the window's has_trans.
 *         Everything else is as today.
 *      GUARANTEED: for an album in which no frame is quantised, a GIF viewer composites the flagged file to the same
 *      canvases, frame by frame, as the file without the bit: a held pixel is replaced only where the canvas already holds
 *      that colour.  Where a frame IS quantised, a held pixel shows an EARLIER frame's rendering of the same source colour
 *      (that frame's own table entry, not this frame's), so such a file does not composite to the flag-less file's canvases.
 *      impgpu_gif_encode_bound holds unchanged: a window is never larger than its frame.
 *      ONE launch more per group than the same call without the bit -- 6, or 9 under IMPGPU_GIF_ENC_QUANTIZE; *launches says
 *      so -- and the same two waits: k_gif_enc_delta runs ahead of k_gif_enc_sets on the same 4096-pixel items (a lane
 *      compares its 16 keys with the previous frame's and leaves 16 held bits; the bounds of the pixels not held are folded
 *      across the wave, then the workgroup, and one lane publishes them with atomicMax: integer and order-free, the same
 *      file on every run).  The later launches read the held bits, never the previous frame.  The host plans the segments
 *      for the whole frame (it cannot know the window without a third wait): the segments behind the window's last pixel
 *      stay empty.  WHERE IT LOSES: an album in which everything changes pays k_gif_enc_delta and a second colour set per
 *      candidate and gains nothing.
 *      MEASURED (profiles/gif_delta_probe.json, one session, flag off -> on; a still background and a 64 x 64
 *      patch that moves): 8 frames at 640x480 2.47 -> 2.30 ms and 3.28 -> 0.46 MB (past 256 colours, with QUANTIZE: 3.07 -> 2.80
 *      ms, 1.20 -> 0.18 MB); 64 albums of 8 frames at 320x240 19.6 -> 10.1 ms, 50.8 -> 9.4 MB (25.1 -> 13.0 ms, 25.3 -> 5.6 MB).
 *      A lone album gains little time: its first frame is written whole and one segment's walk is the call.  Everything
 *      changing: 2.48 -> 2.52 ms (+1.8 %), and the file grows by 0.04 %. ---- */
#define IMPGPU_GIF_ENC_DELTA 2
int impgpu_album_encode_gif_ex2(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment,
                                int flags, unsigned char* out, size_t capacity, size_t* length);
int impgpu_batch_encode_gif_ex2(const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                                const int* loop_counts, int count, int segment, int flags, unsigned char* const* outs,
                                const size_t* capacities, size_t* lengths, int* codes, int* launches);
int impgpu_gif_encode_host_ex2(const unsigned char* const* frames, int count, int width, int height, int channels, int step,
                               const int* time_ms, const int* dispose, int loop_count, int segment, int flags,
                               unsigned char* out, size_t capacity, size_t* length);

/* ---- WEBP ANSWERS out, LOSSLESS, written ON THE DEVICE (opt-in: nothing calls these by default; the broker does not yet).
 *      `format=webp&quality=256..511` asks FreeImage for a lossless file (bit 8 of its flags word is WEBP_LOSSLESS;
 *      impgpu_request_webp_lossless says whether a parsed request does).  The file is deterministic, all-integer and NOT
 *      libwebp's bytes; any VP8L decoder returns exactly the frame's pixels.  THE FILE, completely:
 *      CONTAINER  "RIFF", u32 file size - 8, "WEBP", "VP8L", u32 payload size, the payload, one 0 byte when that size is odd.
 *      BITS  are packed LSB-first, a value's low bit first.  PAYLOAD HEADER: the byte 0x2f, 14 bits width - 1, 14 bits
 *        height - 1, 1 bit alpha_is_used (1 iff the frame has 4 channels and some alpha is not 255; alpha is written
 *        faithfully either way), 3 bits version 0.
 *      PIXELS  are A<<24 | R<<16 | G<<8 | B; a gray frame has R = G = B = v and A = 255, a B,G,R frame has A = 255.
 *      TRANSFORMS, each announced by a 1 bit and 2 bits of type: subtract-green (type 2: R -= G, B -= G mod 256), then the
 *        predictor (type 0), which adds 3 bits IMPGPU_WEBP_TILE_BITS - 2 and its MODE IMAGE; then a 0 bit.  The predictor
 *        works on the green-subtracted image; the residual is pixel - prediction per channel mod 256.
 *      PREDICTIONS  with L, T, TL, TR the left, top, top-left and top-right green-subtracted pixels (TR of the last column
 *        is column 0 of the current row): pixel (0,0) is predicted 0xff000000, the rest of row 0 by L, the rest of column 0
 *        by T; elsewhere the mode of the pixel's tile (tiles of 2^IMPGPU_WEBP_TILE_BITS pixels a side) applies: 0 0xff000000,
 *        1 L, 2 T, 3 TR, 4 TL, 5 Avg2(Avg2(L,TR),T), 6 Avg2(L,TL), 7 Avg2(L,T), 8 Avg2(TL,T), 9 Avg2(T,TR),
 *        10 Avg2(Avg2(L,TL),Avg2(T,TR)), 11 Select, 12 ClampAddSubtractFull(L,T,TL), 13 ClampAddSubtractHalf(Avg2(L,T),TL).
 *        Avg2 is (a+b)>>1 per channel.  Select: with p = L+T-TL per channel, L when sum|p-L| < sum|p-T| over the four
 *        channels, else T.  Full is clamp(L+T-TL) to 0..255; Half(a,b) is clamp(a + (a-b)/2), C division toward zero.
 *      MODE CHOICE  per tile: every mode 0..13 is evaluated over the tile's pixels (the ones whose prediction the edge rules
 *        fix included: they cost the same under every mode); a mode's cost is the sum of min(r, 256-r) over the four
 *        residual channels; the smallest cost wins, a tie goes to the lowest mode.
 *      MODE IMAGE  ceil(w / 2^bits) x ceil(h / 2^bits) pixels 0xff000000 | mode<<8, an entropy-coded image WITHOUT the
 *        meta-prefix bit.
 *      ENTROPY-CODED IMAGE  a 0 bit (no colour cache); for the main image alone a 0 bit (no meta prefix image); five prefix
 *        codes in the order green (alphabet 280), red, blue, alpha (256 each), distance (40); then the pixels in raster order,
 *        each as its green, red, blue, alpha symbol.  No backward references: green symbols 256..279 never occur, and the
 *        distance code is the bits 1,0,0,0 (simple, one symbol, 0).
 *      PREFIX CODES  a code with exactly ONE used symbol is the simple form 1,0,1 and the 8-bit symbol, and its symbols take
 *        no bits.  Every other code (two used symbols included) is the normal form: 0; 4 bits count - 4; `count` 3-bit lengths
 *        of the code-length code in the order 17,18,0,1,2,3,4,5,16,6,7,...,15, count being 19 less the trailing zeros of that
 *        list, at least 4; a 0 bit (no max_symbol); then the lengths of ALL symbols of the alphabet.
 *        LENGTHS are what zlib 1.2.11's build_tree + gen_bitlen (trees.c) give the frequencies: the heap ordered by
 *        (frequency, depth), equal pairs broken by the heap's own layout, at most 15 bits (7 for the code-length code) by
 *        gen_bitlen's repair.  Such a code is complete (Kraft sum 1), which libwebp demands.  Codes are canonical
 *        (gen_codes) and written bit-reversed, as in deflate.
 *        RUNS  the length list is tokenised by zlib's send_tree over the whole alphabet: a run of zeros of 3..10 is 17 and
 *        3 extra bits, of 11..138 is 18 and 7 extra bits; a run of a non-zero length is the length once (unless the run
 *        before it had the same length) and then 16 with 2 extra bits for 3..6 repeats; shorter runs are literal lengths;
 *        a run is cut at 138 zeros, at 7 (6 right after a run of the same length) otherwise.  16 always follows its own length.
 *        The code-length code's frequencies are the tokens' counts.
 *      tests/webp_writer.py writes the same bytes from this paragraph alone.
 *      TAKEN: 1-, 3- and 4-channel single images with sides 1..16384; a window of a parent (step > width x channels) is
 *      read in place.  REFUSED: IMP_ERROR_UNSUPPORTED, *length = 0, nothing written: an album, 2 channels, a larger side.
 *      IMP_ERROR_MALLOC_FAILED: `capacity` is too small; nothing is written, *length is the size needed
 *      (impgpu_webp_encode_bound is always enough) -- and, with *length = 0, a frame whose device block does not fit under
 *      $IMPGPU_STAGE_CAP_MB.  IMP_ERROR_INVALID_ARGS before a device is looked for: NULL arrays with count > 0, a count
 *      outside 0..256, a forced mode above 13.  IMP_ERROR_DEVICE without an env.
 *      SIX launches for a call (for a group under $IMPGPU_STAGE_CAP_MB), whatever it holds: k_webp_modes (a wavefront per
 *      tile sums the 14 costs, exchanged across the wave), k_webp_resid (residual plane; four 256-bin histograms in LDS per
 *      workgroup, added to the frame's: the sums do not depend on the order, so every run gives the same file),
 *      k_webp_codes (a wavefront per frame; five lanes build a code each, one lane strings the header pieces together and
 *      writes the record and the container's sizes), k_webp_measure (the bits of every item of 1024 symbols), k_webp_scan
 *      (64-bit exclusive offsets) and k_webp_emit (an item's codes are ORed into LDS at their bit positions, 32 bits at most at a time; whole dwords
 *      leave by plain stores, an item's first and last dword by an OR into the zeroed file, since a neighbour may share
 *      them).  No kernel walks pixels sequentially.  TWO waits: the records (the lengths), then the files that fit.
 *      MEASURED: (profiles/webp_encode_probe.json, one session, BGRA frames): a lone 640x480 photo-like frame
 *      1.43 ms, a lone 1920x1080 one 2.75 ms, 64 frames of 320x240 4.99 ms -- against 0.11 / 0.53 / 1.72 ms for impgpu_batch_download
 *      of the frames alone and 8.9 / 94.8 / 119 ms for that plus Pillow's lossless save (method 0) on one core.  Files 5 % smaller
 *      than libwebp's method 0 on photo-like frames, 4.3x LARGER on dithered 256-colour frames and no match at all on flat
 *      colour (a bit per pixel against 38 bytes): there are no backward references.  k_webp_codes (five sequential trees per
 *      frame in device memory) is 1.0-1.5 ms of every call; the other five launches together 0.07-0.19 ms. ---- */
#define IMPGPU_WEBP_TILE_BITS 4
int impgpu_image_encode_webp(const impgpu_image* image, unsigned char* out, size_t capacity, size_t* length);
/* diagnostic: forced_modes = one byte 0..13 per tile in raster order, and the chooser is skipped; NULL IS the call above */
int impgpu_image_encode_webp_ex(const impgpu_image* image, const unsigned char* forced_modes, unsigned char* out, size_t capacity,
                                size_t* length);
/* MANY frames (count 0..256) of mixed sizes and channel counts: codes[i] / lengths[i] / the file are exactly the lone
 * call's; a refused frame gets its code alone and changes no other entry.  *launches (may be NULL): the kernels enqueued
 * -- 6 for a call under the stage cap whatever it holds, 0 when no frame was accepted. */
int impgpu_batch_encode_webp(const impgpu_image* const* images, int count, unsigned char* const* outs, const size_t* capacities,
                             size_t* lengths, int* codes, int* launches);
/* a size no file of that geometry exceeds (0: a geometry the calls refuse) */
size_t impgpu_webp_encode_bound(int width, int height, int channels);
/* host, no device: the same file from a frame in host memory (rows `step` bytes apart), made by the launches' own lane code
 * (csrc/imp_webp_enc.h) run one lane after the other.  forced_modes as above (normally NULL). */
int impgpu_webp_encode_host(const unsigned char* frame, int width, int height, int channels, int step,
                            const unsigned char* forced_modes, unsigned char* out, size_t capacity, size_t* length);
/* ---- WEBP ANSWERS, BACKWARD REFERENCES (opt-in flag IMPGPU_WEBP_ENC_BACKREFS on the _flags calls below; without it every
 *      call, byte and launch count above stays what it is).  THE FILE WITH THE FLAG:
 *      THE SAME  container, payload header, transforms, predictions, mode choice and mode image, exactly.  The mode image
 *        gets no backward references; its distance code stays the bits 1,0,0,0.  The prefix-code rules (simple / normal
 *        form, build_tree, send_tree runs) are unchanged and now also serve the green code over all its 280 symbols and the
 *        main image's distance code (alphabet 40, lengths of ALL 40 symbols).
 *      WHAT DIFFERS  is the main image's pixel stream.  The residual plane, in raster order p = 0 .. w*h - 1, is cut into
 *        items of 1024 positions; each item is parsed on its own, greedily, from its first position s to its end
 *        e = min(s + 1024, w*h).
 *        CANDIDATES  k = 1 .. 24 are the first 24 entries of VP8L's distance map, as (xi, yi): (0,1) (1,0) (1,1) (-1,1) (0,2)
 *          (2,0) (1,2) (-1,2) (2,1) (-2,1) (2,2) (-2,2) (0,3) (3,0) (1,3) (-1,3) (3,1) (-3,1) (2,3) (-2,3) (3,2) (-3,2) (0,4)
 *          (4,0).  Candidate k's distance is d_k = xi + yi * w; it is usable at p iff 1 <= d_k <= p.  A match may start at an
 *          item's first position and read residuals of earlier items; it may not run past e.
 *        MATCH LENGTH  L_k(p) is the largest L with p + L <= e and resid[p+i] == resid[p+i-d_k] for all 0 <= i < L (0 when k
 *          is not usable at p); all four channels are compared as one dword; the match may overlap itself, as in any LZ77.
 *        CHOICE  the largest L_k wins, a tie goes to the lowest k.  If the winner is >= IMPGPU_WEBP_MIN_MATCH (3) the token
 *          is a backward reference (length, k) and p advances by the length; otherwise the token is the literal pixel and p
 *          advances by 1.
 *        A LITERAL is coded as above: its green, red, blue and alpha symbols.  A BACKWARD REFERENCE is, in this order, the
 *          green code's symbol 256 + s_len, the length's extra bits, the distance code's symbol s_dist, its extra bits.
 *          The length (3..1024) and the plane code k (1..24) both use VP8L's prefix coding of a value v >= 1: v <= 4 gives
 *          symbol v - 1 and no extra bits; otherwise, with u = v - 1, hb = floor(log2 u) and sb = (u >> (hb-1)) & 1, the
 *          symbol is 2*hb + sb and there are hb - 1 extra bits of value u & ((1 << (hb-1)) - 1), written LSB-first.  (The
 *          decoder: a symbol below 4 stands for sym + 1; otherwise eb = (sym-2) >> 1 and v = ((2 + (sym&1)) << eb) + bits(eb)
 *          + 1.)  Lengths use symbols 2..19, distances 0..8; a plane code above 120, a colour cache and a meta prefix image
 *          never occur.
 *        HISTOGRAMS  count tokens: a literal its four symbols, a reference one green symbol 256.. and one distance symbol.
 *        DISTANCE CODE  no used symbol: the bits 1,0,0,0 as above; one used symbol: the simple form 1,0,1 and the 8-bit
 *          symbol; otherwise the normal form over 40 symbols.
 *        CONSEQUENCES  a frame in which no position finds a match of 3 is byte for byte the flag-less file; position 0 is
 *          always a literal (so no code of the main image is unused but the distance code); 60 bits still bound a
 *          position: 15 + 8 + 15 + 3 for a reference.
 *      tests/webp_lz_writer.py writes the same bytes from this paragraph alone (and webp_writer's rules).
 *      SEVEN launches with the flag, two waits: k_webp_resid writes the residual plane and counts nothing; k_webp_parse, a
 *      workgroup per item of 1024 positions, follows it: per candidate the item's equality bits go to LDS as 32 words from
 *      wave ballots, a position's L_k is the distance to the next zero bit found by word operations, every position notes
 *      where its token would end, and the token starts -- the positions reached from s -- are marked by pointer doubling (ten
 *      jump tables in LDS, applied from the highest power down); the tokens go to a TOKEN PLANE (a dword a position: 0
 *      covered, a literal marker, or length | k << 16) and into histograms staged in LDS (green over 280, red, blue, alpha,
 *      distance over 40, the total of the extra bits in 64 bits), added once a workgroup; the sums do not depend on the
 *      order, so every run gives the same file.  k_webp_codes gives a sixth lane the distance code; k_webp_measure / _scan /
 *      _emit keep their shape, a covered position being 0 bits and a reference four parts of at most 15, 8, 15 and 3 bits.
 *      The device block grows by the token plane (4 bytes a pixel) and a second work area a frame; the groups under
 *      $IMPGPU_STAGE_CAP_MB count both.
 *      WHAT IT WINS AND WHAT NOT (profiles/webp_lz_sizes.json, 320x240 B,G,R, against the flag-less file / libwebp method 0):
 *      flat colour 152 B / 28 852 B / 38 B; a synthetic screenshot 708 / 29 124 / 342; a Bayer-dithered frame 22 610 / 41 710 /
 *      12 474; a photo-like frame 119 720 / 119 720 / 125 710 -- no match of 3 in sensor noise, the flag-less file.  Matches are
 *      confined to an item of 1024 positions and to 24 neighbours, and there is no colour cache: libwebp stays 2x ahead on
 *      graphics and dither.  MEASURED (profiles/webp_lz_probe.json, one session, flag off / on alternating, BGRA): a lone
 *      640x480 frame 1.44 / 1.48 ms photo-like, 0.78 / 0.84 dithered, 0.49 / 0.56 flat; 1920x1080 3.05 / 3.07, 2.26 / 2.27,
 *      1.60 / 1.69; 64 frames of 320x240 5.16 / 5.40, 4.64 / 4.75, 3.91 / 3.66.  The flagged call is BEHIND the flag-less one by
 *      0.01-0.24 ms everywhere but the last: k_webp_parse costs 42-48 / 111-125 / 228-250 us, k_webp_codes 20-50 us more, and
 *      k_webp_codes' 0.3-1.4 ms is still most of every call.  What crosses the link shrinks with the file: 1.7 MB -> 0.8 MB
 *      (1080p dithered), 778 KB -> 2.6 KB (1080p flat). ----
 * the calls with `flags`: 0 IS the call above (same bytes, same codes, six launches); IMPGPU_WEBP_ENC_BACKREFS writes the file
 * of the paragraph above in seven launches.  An unknown flag bit: IMP_ERROR_INVALID_ARGS before a device is looked for.
 * Refusals and the IMP_ERROR_MALLOC_FAILED contract are the ones above.  forced_modes: normally NULL. */
#define IMPGPU_WEBP_ENC_BACKREFS 1
#define IMPGPU_WEBP_MIN_MATCH 3
int impgpu_image_encode_webp_flags(const impgpu_image* image, int flags, const unsigned char* forced_modes, unsigned char* out, size_t capacity,
                                   size_t* length);
int impgpu_batch_encode_webp_flags(const impgpu_image* const* images, int count, int flags, unsigned char* const* outs, const size_t* capacities,
                                   size_t* lengths, int* codes, int* launches);
int impgpu_webp_encode_host_flags(const unsigned char* frame, int width, int height, int channels, int step, int flags,
                                  const unsigned char* forced_modes, unsigned char* out, size_t capacity, size_t* length);
/* impgpu_webp_encode_bound with the flags' longer distance-code header included */
size_t impgpu_webp_encode_bound_flags(int width, int height, int channels, int flags);
/* 1 when the request's answer format resolves to webp (format=, else the extension) and its parsed quality has bit 8 set
 * (256..511: FreeImage's WEBP_LOSSLESS); otherwise 0.  A pure accessor: the parse and its error codes are unchanged. */
int impgpu_request_webp_lossless(const impgpu_request* request);

/* ---- LOSSY WEBP ANSWERS out, written ON THE DEVICE (opt-in: nothing calls these by default; the broker does not yet).
 *      `format=webp` with a quality of 0..100 asks for a lossy file (impgpu_request_webp_quality says which).  The file is
 *      a VP8 key frame restricted to tools that run in parallel and can be tested exactly; it is deterministic, all-integer
 *      and NOT libwebp's bytes.  libwebp decodes it to exactly the encoder's own reconstruction.  Names of syntax elements
 *      and "the standard ..." refer to RFC 6386; the standard tables are include/impgpu_vp8_tables.h.  THE FILE, completely:
 *      CONTAINER  "RIFF", u32 file size - 8, "WEBP", then chunks: a tag, u32 size, the body, one 0 byte when the size is
 *        odd.  A 1- or 3-channel frame, or a 4-channel frame whose alpha is 255 everywhere, has the one chunk "VP8 ".  A
 *        4-channel frame with any other alpha has "VP8X" (10 bytes: 0x10, 0, 0, 0, u24 width - 1, u24 height - 1), then
 *        "ALPH" (the byte 0 -- no pre-processing, no filter, no compression -- and width x height raw alpha bytes), then
 *        "VP8 ".  Sides run 1..16383.
 *      COLOUR  with R, G, B of a pixel (gray: R = G = B): Y = (16839 R + 33059 G + 6420 B + (16<<16) + (1<<15)) >> 16.
 *        U and V come from the SUMS R, G, B of a 2x2 cell: U = (-9719 R - 19081 G + 28800 B + (128<<18) + (1<<17)) >> 18,
 *        V = (28800 R - 24116 G - 4684 B + (128<<18) + (1<<17)) >> 18, arithmetic shifts, clipped to 0..255.  A cell at an odd
 *        right or bottom edge repeats its last column or row.  The planes are padded to whole macroblocks (16x16 Y, 8x8 U
 *        and V) by repeating the last sample of a row and then the last row.
 *      VP8 CHUNK  the 3-byte frame tag (u24: bit 0 = 0 key frame, bits 1..3 version 0, bit 4 show_frame 1, bits 5..23 the
 *        first partition's size), 0x9d 0x01 0x2a, u16 width, u16 height (scale bits 0), the first partition, then u24 sizes
 *        of all token partitions but the last, then the token partitions.
 *      BOOLEAN CODER  the standard one (section 7.3: range 255, bottom 0, bit_count 24; split = 1 + (((range - 1) * prob)
 *        >> 8); a carry is added into the bytes already written) with that section's flush, which always writes 4 more
 *        bytes.  A literal of n bits is its bits from the highest down at probability 128.  Each partition is one coder.
 *      FIRST PARTITION  literals: colour space 0 (1 bit), clamping type 0 (1), segmentation_enabled 0 (1), filter type 0
 *        (1), loop filter level 0 (6), sharpness 0 (3), loop_filter_adj_enable 0 (1), log2 of the partition count (2), the
 *        quantiser index qi (7), five absent quantiser deltas (0, 1 bit each), refresh_entropy_probs 0 (1); then 1056 flags
 *        0, one per coefficient probability, each coded with its update probability; mb_no_coeff_skip 1 (1) and
 *        prob_skip_false (8) = clamp(1..255, (256 * (MBs - skipped) + MBs/2) / MBs).  Then per macroblock in raster order:
 *        the skip flag at prob_skip_false; a 1 at 145 (not B_PRED); the luma mode: at 156 a 0 then at 163 DC 0 / V 1, or
 *        a 1 then at 128 H 0 / TM 1; the chroma mode: DC is 0 at 142; V is 1 at 142, 0 at 114; H is 1, 1, 0 at 183; TM is
 *        1, 1, 1.
 *      PARTITIONS  P = the largest of 1, 2, 4, 8 that does not exceed the number of macroblock rows; row r's tokens go to
 *        partition r mod P, rows and macroblocks in raster order.
 *      QUANTISER  qi = 127 - (127 * quality + 50) / 100.  With dc[] and ac[] the standard lookups at qi the steps are:
 *        Y1 AC ac; Y2 DC 2 dc; Y2 AC max(8, ac * 155 / 100); chroma DC min(132, dc); chroma AC ac (Y1 DC is not coded:
 *        every macroblock has a Y2 block).  level = sign(c) * min(2047, (|c| + q/2) / q); a de-quantised value is level * q.
 *      PREDICTION  modes DC, V, H, TM (numbered 0..3 in this library) for the 16x16 luma block and, one mode for both, the
 *        8x8 U and V blocks; never B_PRED.  A prediction reads the RECONSTRUCTED samples above (A), to the left (L) and at
 *        the corner (C): the row above the frame is 127, its corner too; the column left of the frame is 129, and so is the
 *        corner of the first macroblock of every row below the first.  V is A[x]; H is L[y]; TM is clip(A[x] + L[y] - C);
 *        DC is (sum A + sum L + n) >> log2(2n) inside (n = 16 or 8), (sum + n/2) >> log2(n) over the one side that exists in
 *        the first row or column, and 128 for the first macroblock.
 *      MODE CHOICE  luma: the mode with the smallest sum of squared differences between prediction and source over the
 *        macroblock wins, a tie goes to the first of DC, V, H, TM.  Chroma likewise over the sum of both planes.
 *      FORWARD TRANSFORMS  of the differences d (source - prediction) of a 4x4 block, rows first: a0 = d0 + d3, a1 = d1 + d2,
 *        a2 = d1 - d2, a3 = d0 - d3; t0 = (a0 + a1) * 8, t1 = (a2 * 2217 + a3 * 5352 + 1812) >> 9, t2 = (a0 - a1) * 8,
 *        t3 = (a3 * 2217 - a2 * 5352 + 937) >> 9.  Then columns of t, with the same a0..a3: c0 = (a0 + a1 + 7) >> 4,
 *        c1 = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0), c2 = (a0 - a1 + 7) >> 4, c3 = (a3 * 2217 - a2 * 5352 +
 *        51000) >> 16, c_k being row k of the block's coefficients.  The 16 luma blocks' first coefficients (their DCs), in
 *        the blocks' raster order, form the 4x4 Y2 input; its Walsh-Hadamard transform, rows first: a0 = i0 + i2, a1 = i1 + i3, a2 = i1 - i3, a3 = i0 - i2;
 *        t = a0 + a1, a3 + a2, a3 - a2, a0 - a1; then columns: a0 = t0 + t2, a1 = t1 + t3, a2 = t1 - t3, a3 = t0 - t2 (t_k
 *        row k) and the outputs (a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1 as rows 0..3.
 *      RECONSTRUCTION  is the decoder's: the standard inverse WHT of the de-quantised Y2 block gives the luma blocks' DCs
 *        (used as they are); the standard inverse DCT (20091 / 35468, section 14.3) of each de-quantised block is added to the
 *        prediction and clamped to 0..255.
 *      SKIP  a macroblock whose 25 blocks have only zero levels is skipped: no tokens, all its context flags 0.
 *      TOKENS  of a coded macroblock: the Y2 block (type 1), the 16 luma blocks in raster order (type 0, from position 1),
 *        the 4 U and the 4 V blocks (type 2): the standard token tree with the DEFAULT coefficient probabilities, the
 *        standard bands, zigzag and category extra bits, the sign at 128; a block's context is the number of its left and
 *        upper neighbours of the same kind (in this macroblock or the next one over, 0 outside the frame) that coded a
 *        non-zero level; the context after a token is 0, 1 or 2 for a zero, a one, anything larger.
 *      tests/webp_vp8_writer.py writes the same bytes from this paragraph alone.
 *      TAKEN: 1-, 3- and 4-channel single images with sides 1..16383, quality 0..100; a window of a parent (step > width x
 *      channels) is read in place.  REFUSED: IMP_ERROR_UNSUPPORTED, *length = 0, nothing written: an album, 2 channels, a
 *      larger side -- and a frame whose first partition outgrows the format's 19-bit size or a token partition its 24 bits
 *      (about 300 000 macroblocks).  IMP_ERROR_MALLOC_FAILED: `capacity` is too small; nothing is written, *length is the
 *      size needed (impgpu_webp_lossy_encode_bound is always enough: it is the worst case of the token tree, about 8 KB a
 *      macroblock) -- and, with *length = 0, a frame whose device block does not fit under $IMPGPU_STAGE_CAP_MB.
 *      IMP_ERROR_INVALID_ARGS before a device is looked for: a quality outside 0..100, NULL arrays with count > 0, a
 *      count outside 0..256.  IMP_ERROR_DEVICE without an env.
 *      FIVE launches for a call (for a group under $IMPGPU_STAGE_CAP_MB), whatever it holds: k_vp8_planes (padded Y, U, V
 *      and the alpha plane, a gather per sample), k_vp8_recon (a workgroup per frame, a wavefront per macroblock row in
 *      flight -- 8, fewer past 7168 pixels a row -- each one macroblock behind the row above; progress counters and the border rows in LDS; the 64 lanes share
 *      a macroblock's mode costs, 25 transforms, quantiser and reconstruction; it leaves the levels and a word of modes
 *      and non-zero flags per macroblock), k_vp8_tokens (a lane per macroblock writes its (probability, bit) records),
 *      k_vp8_bool (a lane per frame and partition walks its records through the boolean coder, carries resolved in its
 *      own output; a ninth lane codes the first partition) and k_vp8_pack (sizes, frame tag, partition table, chunks and
 *      the pieces into the answer).  TWO waits: the records (the lengths), then the files that fit.
 *      MEASURED (profiles/webp_lossy_probe.json, one session, photo-like BGRA frames, quality 75): 64
 *      frames of 320x240 2.93 ms (two groups), a lone 640x480 frame 4.08 ms, a lone 1920x1080 one 24.3 ms -- against 1.33 /
 *      0.09 / 0.41 ms for impgpu_batch_download of the frames alone and 63.6 / 3.92 / 24.4 ms for that plus Pillow's lossy
 *      save at method 0 on one core (233 / 14.1 / 93.5 ms at method 4).  A lone frame only ties libwebp's fastest setting:
 *      k_vp8_recon and k_vp8_bool are sequential and take half the call each (1.9 + 2.1 ms at 640x480, 11.9 + 12.7 ms at
 *      1080p); the other three launches together are under 0.35 ms.  Files are about libwebp's size at equal quality and
 *      1.4x / 2.2x / 3.2x larger at equal PSNR (quality 50 / 75 / 90, profiles/webp_lossy_sizes.json): no B_PRED, default
 *      probabilities, no loop filter, plain rounding. ---- */
int impgpu_image_encode_webp_lossy(const impgpu_image* image, int quality, unsigned char* out, size_t capacity, size_t* length);
/* MANY frames (count 0..256) of mixed sizes, channel counts and qualities: codes[i] / lengths[i] / the file are exactly the
 * lone call's; a refused frame gets its code alone and changes no other entry.  *launches (may be NULL): the kernels
 * enqueued -- 5 for a call under the stage cap whatever it holds, 0 when no frame was accepted. */
int impgpu_batch_encode_webp_lossy(const impgpu_image* const* images, int count, const int* qualities, unsigned char* const* outs,
                                   const size_t* capacities, size_t* lengths, int* codes, int* launches);
/* a size no file of that geometry exceeds (0: a geometry the calls refuse) */
size_t impgpu_webp_lossy_encode_bound(int width, int height, int channels);
/* host, no device: the same file from a frame in host memory (rows `step` bytes apart), made by the launches' own lane code
 * (csrc/imp_webp_lossy.h) run one lane after the other. */
int impgpu_webp_lossy_encode_host(const unsigned char* frame, int width, int height, int channels, int step, int quality,
                                  unsigned char* out, size_t capacity, size_t* length);
/* the same, and what the encoder decided, for the tests (each may be NULL): per macroblock in raster order `modes` 2 bytes
 * (luma, chroma), `levels` 400 shorts (25 blocks -- 16 Y, 4 U, 4 V, Y2 -- of 16 levels in raster order); the reconstructed
 * planes padded to whole macroblocks (16 mbw x 16 mbh, and half that a side for U and V). */
int impgpu_webp_lossy_encode_host_ex(const unsigned char* frame, int width, int height, int channels, int step, int quality,
                                     unsigned char* out, size_t capacity, size_t* length, unsigned char* modes, short* levels,
                                     unsigned char* recon_y, unsigned char* recon_u, unsigned char* recon_v);
/* -1 unless the request's answer format resolves to webp (format=, else the extension) with bit 8 of its parsed quality
 * clear; otherwise the lossy quality: an absent quality or 0 is 75, one above 100 is 100.  (The mapping is this
 * library's.)  A pure accessor: the parse and its error codes are unchanged. */
int impgpu_request_webp_quality(const impgpu_request* request);

/* ---- WEBP UPLOADS in, LOSSLESS, decoded ON THE DEVICE (opt-in: nothing calls these by default; the broker only with
 *      --webp-accept lossless).  THE FRAME is what the reference's route gives for the same file -- FreeImage's WebP plugin,
 *      ConvertTo32Bits, LoadSingle (advancedio.c:276-318), then impgpu_image_upload_fi32: 4 channels, top-down, B,G,R,A; A is
 *      the decoded alpha when the VP8L header's alpha_is_used bit is set and 255 otherwise (Pillow: mode RGBA with the bit,
 *      RGB without).  `channels` is always 4.
 *      TAKEN: a RIFF / WEBP file whose image is ONE VP8L chunk, alone or inside a VP8X container (ICCP, EXIF, XMP and unknown
 *      chunks are skipped, as libwebp's plain decode skips them); version 0; any width and height the format can say (16384
 *      a side) up to IMPGPU_WEBP_DEC_MAX_PIXELS pixels (8192 x 8192); all of VP8L: the four transforms, each at most once, in
 *      any order; colour indexing with 1, 2, 4 and 8 pixels a value (an index past the palette is 0x00000000); the colour
 *      cache at 1..11 bits; the entropy image with any number of prefix-code groups; normal and simple prefix codes with the
 *      repeat codes 16, 17, 18 and max_symbol; backward references with all 120 mapped distance codes and the plain ones
 *      beyond, a mapped distance below 1 being 1.
 *      IMP_ERROR_UNSUPPORTED (decode on the host as before): a VP8 (lossy) image, ANIM / ANMF, ALPH, a version other than 0,
 *      more pixels than the limit, or not a WebP at all.
 *      IMP_ERROR_DECODE_FAILED: a chunk size that runs past the file; a transform that appears twice; a colour-cache size
 *      outside 1..11; a prefix code libwebp refuses (no symbol at all, over-subscribed, incomplete -- but exactly one symbol
 *      of length 1..14 is the code of zero bits); a repeat past the alphabet, max_symbol past it; a colour-cache index when
 *      no cache exists; a distance before the first pixel; a match that runs past the image; a stream that runs past its
 *      chunk (anywhere: in the headers, the sub-images or the pixels).  Judged per file: a bad file changes no other file's
 *      result.
 *      HOW: the host reads what lies in front of the main image's pixel stream (the container, the header, the transforms
 *      with their small sub-images, the cache size, the entropy image, every group's code lengths) with the lanes' own
 *      decoder; the compressed bytes, the code lengths, the sub-images and a descriptor per file go up in ONE upload a group
 *      (one pinned block, one device block).  IMPGPU_WEBP_DEC_LAUNCHES (3) kernels a group, whatever it holds:
 *      k_webp_dec_tables (a wavefront per prefix code builds and judges every group's lookup tables, in global memory),
 *      k_webp_dec_pixels (a wavefront per file, in rounds: stage words, decode symbols wave-uniformly into a token list,
 *      emit in token order -- colour-cache tokens are resolved in token order by one lane, not side by side), and
 *      k_webp_dec_inverse (a workgroup per file undoes the transforms last to first, the predictor with rows skewed two
 *      pixels apart, and writes B,G,R,A).  A call is cut into groups under $IMPGPU_STAGE_CAP_MB like the other batch calls.
 *      ONE wait per call: for the files' status words.
 *      MEASURED (profiles/webp_decode_probe.json, tools/webp_decode_probe.py; one session, Pillow-encoded files; the call against
 *      Pillow's decode of the same file on one core + impgpu_image_upload): a lone 640x480 file 201.5 / 4.5 ms photo-like,
 *      60.8 / 2.3 dithered 256-colour, 0.58 / 1.24 flat; a lone 1920x1080 file 1490 / 30.8, 471 / 15.1, 5.7 / 8.1; 64 files of
 *      320x240 54.8 / 75.0, 20.1 / 35.6, 0.92 / 21.1.  A wave on a sequential bit stream LOSES to the host for a lone file, by
 *      27-48x on everything but flat colour: k_webp_dec_pixels is 97-99 % of those calls (199.3 of 201.5 ms: 0.65 us a
 *      literal pixel, four dependent table reads), k_webp_dec_tables 46-73 us, k_webp_dec_inverse 0.4-2.1 ms at 640x480 and
 *      4.9-15.4 ms at 1920x1080, the host front 0.02-0.22 ms a file.  The files of a call decode side by side, a wave each, so
 *      a call takes what its slowest file takes: 64 files are AHEAD of the host route (1.4x photo-like, 1.8x dithered, 23x
 *      flat), and the crossover lies near 45 photo-like or 35 dithered files of 320x240 a call. ---- */
#define IMPGPU_WEBP_DEC_MAX_PIXELS (1 << 26)
#define IMPGPU_WEBP_DEC_LAUNCHES 3
#define IMPGPU_WEBP_DEC_INFO_WORDS 8
/* the feature word, info[0] of impgpu_webp_decode_host: what the file uses (the tests prove their coverage with it) */
#define IMPGPU_WEBP_DEC_F_PREDICTOR      0x0001
#define IMPGPU_WEBP_DEC_F_COLOR          0x0002
#define IMPGPU_WEBP_DEC_F_SUB_GREEN      0x0004
#define IMPGPU_WEBP_DEC_F_INDEXING       0x0008
#define IMPGPU_WEBP_DEC_F_CACHE          0x0010   /* a colour cache, in the main image or a sub-image */
#define IMPGPU_WEBP_DEC_F_GROUPS         0x0020   /* more than one prefix-code group */
#define IMPGPU_WEBP_DEC_F_BACKREF        0x0040
#define IMPGPU_WEBP_DEC_F_SIMPLE         0x0080   /* a simple prefix code */
#define IMPGPU_WEBP_DEC_F_DIST_ABOVE_24  0x0100   /* a distance code above 24 */
#define IMPGPU_WEBP_DEC_F_DIST_CLAMPED   0x0200   /* a mapped distance below 1 that became 1 */
#define IMPGPU_WEBP_DEC_F_BUNDLE_1       0x0400   /* colour indexing, one pixel a value (more than 16 colours) */
#define IMPGPU_WEBP_DEC_F_BUNDLE_2       0x0800   /* two pixels a value (5..16 colours) */
#define IMPGPU_WEBP_DEC_F_BUNDLE_4       0x1000   /* four (3..4 colours) */
#define IMPGPU_WEBP_DEC_F_BUNDLE_8       0x2000   /* eight (1..2 colours) */
#define IMPGPU_WEBP_DEC_F_ALL            0x3fff
/* The geometry alone: IMP_OK, or the refusal / failure the container and the five header bytes already show.  Host only. */
int impgpu_webp_info(const unsigned char* blob, size_t size, int* width, int* height, int* channels);
int impgpu_image_decode_webp(const unsigned char* blob, size_t size, impgpu_image** out);
/* codes[i] / images[i] are what the single-file call returns alone (images[i] = NULL unless codes[i] == IMP_OK).
 * IMP_ERROR_INVALID_ARGS = a NULL array or count outside 0..256, before any device is looked for; IMP_ERROR_DEVICE without
 * an env (every codes[i] says so too); otherwise IMP_OK with the verdicts in codes[].  *launches (may be NULL): the
 * kernels launched, IMPGPU_WEBP_DEC_LAUNCHES a group that holds a file the host front took. */
int impgpu_batch_decode_webp(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_image** images, int* codes, int* launches);
/* The same decoder with no device: the lanes' code, one lane after the other.  Writes the B,G,R,A frame (width * 4 bytes a
 * row) into out[0, capacity); *width / *height are set once the header is read; IMP_ERROR_MALLOC_FAILED = capacity is
 * smaller than width * height * 4 (nothing written).  info (may be NULL) receives IMPGPU_WEBP_DEC_INFO_WORDS ints: [0] the
 * feature word, [1] prefix-code groups, [2] the main image's cache bits, [3] transforms, [4] the coded width, [5] the
 * main image's status word (0 complete, 1 damaged, 2 ran past the chunk), [6] the rounds the main image took (a round ends
 * at 512 tokens or where the 512 staged words run low), [7] the longest code length among the main image's codes. */
int impgpu_webp_decode_host(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, int* width, int* height, int* info);

/* ---- WEBP UPLOADS in, LOSSY (a VP8 key frame), decoded ON THE DEVICE (opt-in twice: the _ex calls below, and in them the
 *      IMPGPU_WEBP_ACCEPT_LOSSY bit of `accept`; the broker only with --webp-accept all).  accept == 0 IS the call without
 *      _ex: the same frames, codes and launch counts, a lossy file still IMP_ERROR_UNSUPPORTED.  With the bit set a call may
 *      mix lossless, lossy, refused and damaged files in any order; each is judged on its own.
 *      THE FRAME is what the reference's route gives for the file -- FreeImage's WebP plugin, ConvertTo32Bits, LoadSingle,
 *      impgpu_image_upload_fi32: 4 channels, top-down, B,G,R,A with A = 255 -- libwebp's default decode (fancy chroma
 *      upsampling, no dithering), byte for byte what Pillow's libwebp returns as mode RGB.  Where libwebp and RFC 6386
 *      differ libwebp is followed: the edge values 127 / 129, the above-right samples of the rightmost macroblock, the 16-bit
 *      storage of de-quantised coefficients (and the 16-bit lanes of its inverse DCT for blocks past three coefficients:
 *      "libwebp" here is its x86 SSE2 build, the one Pillow ships; a NEON or plain-C build may differ from it, and so from
 *      this decoder, on streams whose coefficients leave 16 bits -- no encoder writes such values),
 *      frame level 0 switching the filter off whatever the segments say, the clamp and scale bits ignored.
 *      TAKEN: a RIFF / WEBP file whose image is ONE `VP8 ` chunk, alone or inside VP8X without ALPH and animation (ICCP,
 *      EXIF, XMP and unknown chunks are skipped); all of a key frame: versions 0..3; any size up to 16383 a side under
 *      IMPGPU_WEBP_DEC_MAX_PIXELS, multiples of 16 or not; 1, 2, 4 and 8 token partitions, empty ones included (a size in
 *      the table that runs past the chunk is cut to it, as libwebp does); segmentation with and without a map update,
 *      absolute or delta values; the five quantiser deltas, indices clamped to 0..127; coefficient probability updates;
 *      mb_no_coeff_skip 0 and 1; the four 16x16 and chroma modes, B_PRED with the ten sub-block modes; every token category
 *      up to DCT_CAT6; both loop filters at levels 0..63 and sharpness 0..7 with the key frame's high-edge-variance
 *      thresholds; mode_ref_lf_delta; the inner-edge rule.
 *      IMP_ERROR_UNSUPPORTED (decode on the host as before): ALPH, ANIM / ANMF, an inter frame (libwebp: "Not a key frame",
 *      VP8_STATUS_UNSUPPORTED_FEATURE), show_frame 0 ("Frame not displayable", the same status), more pixels than the limit,
 *      not a WebP.
 *      IMP_ERROR_DECODE_FAILED: a `VP8 ` chunk (or any chunk in front of the image) whose size runs past the file -- with the
 *      bit set the four calls agree on that; without it such a file is IMP_ERROR_UNSUPPORTED as in the calls without _ex,
 *      which refuse the chunk by its name before they look at its size; a bad start code (VP8_STATUS_BITSTREAM_ERROR); a version past 3 (libwebp answers "Incorrect
 *      keyframe parameters" before any pixel: a stream no decoder of this format reads, so a failure here, not a route to
 *      the host); a width or height of 0; a first partition or a partition table that runs past the chunk, a last
 *      partition of no bytes (VP8_STATUS_NOT_ENOUGH_DATA / SUSPENDED); a frame header that runs off the first partition; a
 *      partition the decoder runs off the end of (NOT_ENOUGH_DATA).  The last follows libwebp's rule exactly: the end is
 *      looked at per macroblock (per macroblock row for the first partition), and failure comes only once a byte past the
 *      end HAD to be loaded -- so a file whose last partition lost its 1..3 bytes of flush still decodes to the same frame.
 *      HOW: the host reads the container, the frame tag, the frame header and the partition table (imp_vp8_dec_host.h, with
 *      the lanes' boolean decoder); a descriptor and the chunk's bytes per file go up in the group's ONE upload, beside the
 *      lossless files' blocks.  IMPGPU_WEBP_DEC_LOSSY_LAUNCHES (3) kernels a group that holds a lossy file, whatever else it
 *      holds (a group with a lossless file adds IMPGPU_WEBP_DEC_LAUNCHES; a group of one kind launches that kind's only):
 *      k_vp8_dec_recon (a workgroup per file; ONE lane walks the macroblocks in raster order: modes from the first
 *      partition, tokens from the row's partition, prediction and inverse transforms into padded planes -- everything a
 *      macroblock depends on is that lane's own earlier work, so nothing is waited for), k_vp8_dec_filter (a workgroup per
 *      file: macroblocks in raster order, as the result depends on it; the 16 + 8 + 8 lines of an edge side by side, eight
 *      barrier-separated steps a macroblock) and k_vp8_dec_frame (fully parallel: upsample, convert, crop).  Every loop
 *      over stream data is bounded by the partition's size, 16 coefficients a block and the macroblock count: a damaged file
 *      sets its status word, writes only its own planes and cannot hang.  ONE wait per call.
 *      MEASURED (profiles/webp_lossy_decode_probe.json, tools/webp_lossy_decode_probe.py; one session, Pillow-encoded files at
 *      quality 75; the call against Pillow's decode of the same file on one core + impgpu_image_upload, medians after a
 *      warm-up): a lone 640x480 file 113.4 / 1.9 ms photo-like, 283.3 / 4.2 dithered, 69.8 / 1.4 flat; a lone 1920x1080 file
 *      777 / 12.6, 1931 / 29.1, 468 / 10.1; 64 files of 320x240 30.0 / 32.8, 76.4 / 70.8, 18.4 / 24.3; the host front 0.01-0.02
 *      ms a file.  One lane on sequential boolean streams LOSES to the host for a lone file by 46-67x.  The files of a call
 *      decode side by side, so a call takes what its slowest file takes, and the crossover lies near 64 files of 320x240 a
 *      call (ahead 1.1x photo-like and 1.3x flat there, behind 1.08x dithered).  Per kernel (a separate rocprofv3 --kernel-trace
 *      run of the same cases): k_vp8_dec_recon is 91-98 % of every call (640x480: 102.9 / 276.6 / 66.2 ms; 1920x1080: 717 /
 *      1937 / 438), k_vp8_dec_filter 2.3-7.0 ms at 640x480 and 16-51 ms at 1920x1080, k_vp8_dec_frame 0.02-0.09 ms.  It takes decode work off the workers' cores; it does not answer a lone request sooner. ---- */
#define IMPGPU_WEBP_ACCEPT_LOSSY 1
#define IMPGPU_WEBP_DEC_LOSSY_LAUNCHES 3
/* the feature word of a lossy file, info[0] of impgpu_webp_decode_host_ex */
#define IMPGPU_VP8_DEC_F_SEGMENTS     0x000001
#define IMPGPU_VP8_DEC_F_MAP_UPDATE   0x000002
#define IMPGPU_VP8_DEC_F_DELTA_VALUES 0x000004   /* segment values added to the frame's */
#define IMPGPU_VP8_DEC_F_SIMPLE       0x000008   /* the simple loop filter, at a level above 0 */
#define IMPGPU_VP8_DEC_F_NORMAL       0x000010
#define IMPGPU_VP8_DEC_F_SHARPNESS    0x000020
#define IMPGPU_VP8_DEC_F_LF_DELTA     0x000040
#define IMPGPU_VP8_DEC_F_PARTS2       0x000080
#define IMPGPU_VP8_DEC_F_PARTS4       0x000100
#define IMPGPU_VP8_DEC_F_PARTS8       0x000200
#define IMPGPU_VP8_DEC_F_BPRED        0x000400
#define IMPGPU_VP8_DEC_F_PROB_UPDATE  0x000800
#define IMPGPU_VP8_DEC_F_SKIP_OFF     0x001000   /* mb_no_coeff_skip 0 */
#define IMPGPU_VP8_DEC_F_DQ_Y1DC      0x002000   /* a quantiser delta other than 0: y dc, y2 dc, y2 ac, uv dc, uv ac */
#define IMPGPU_VP8_DEC_F_DQ_Y2DC      0x004000
#define IMPGPU_VP8_DEC_F_DQ_Y2AC      0x008000
#define IMPGPU_VP8_DEC_F_DQ_UVDC      0x010000
#define IMPGPU_VP8_DEC_F_DQ_UVAC      0x020000
#define IMPGPU_VP8_DEC_F_CAT6         0x040000
#define IMPGPU_VP8_DEC_F_CROP_W       0x080000   /* a width that is no multiple of 16 */
#define IMPGPU_VP8_DEC_F_CROP_H       0x100000
#define IMPGPU_VP8_DEC_F_ALL          0x1fffff
#define IMPGPU_VP8_DEC_MODES_ALL      0x3ffff    /* info[1]: 16x16 modes in bits 0..3, chroma 4..7, sub-block 8..17 (libwebp's order) */
/* The calls above with an accept mask.  For a lossy file impgpu_webp_decode_host_ex fills info[] with: [0] the feature
 * word above, [1] the masks of the modes met, [2] token partitions, [3] macroblock columns, [4] macroblock rows, [5] the
 * status word (0 complete, 1 ran off a partition), [6] 0, [7] 1 (a lossless file leaves 0 there). */
int impgpu_webp_info_ex(const unsigned char* blob, size_t size, int accept, int* width, int* height, int* channels);
int impgpu_image_decode_webp_ex(const unsigned char* blob, size_t size, int accept, impgpu_image** out);
int impgpu_batch_decode_webp_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept, impgpu_image** images, int* codes, int* launches);
int impgpu_webp_decode_host_ex(const unsigned char* blob, size_t size, int accept, unsigned char* out, size_t capacity, int* width, int* height, int* info);

/* ---- WEBP UPLOADS in, LOSSY WITH ALPHA (VP8X + ALPH + `VP8 `), decoded ON THE DEVICE (opt-in three times: the _ex calls,
 *      IMPGPU_WEBP_ACCEPT_LOSSY and with it the IMPGPU_WEBP_ACCEPT_ALPHA bit of `accept`; the broker only with
 *      --webp-accept alpha).  The bit means something only together with IMPGPU_WEBP_ACCEPT_LOSSY: accept 2 is accept 0, and
 *      accept 0 / 1 and the calls without _ex give every frame, code and launch count they gave without it (such a file is
 *      IMP_ERROR_UNSUPPORTED there).  These are the files libwebp, Pillow and impgpu_image_encode_webp_lossy (on a 4-channel
 *      frame) write for cut-outs, stickers and logos.
 *      THE FRAME: B,G,R are byte for byte those of the file's `VP8 ` chunk decoded alone; byte 3 is the alpha plane --
 *      what Pillow's libwebp returns as mode RGBA.
 *      THE ALPH CHUNK: a header byte -- bits 0-1 the method (0: w * h raw bytes follow, bytes behind them are ignored; 1: a
 *      VP8L image stream WITHOUT its five header bytes, w x h the frame's, whose green channel is the plane), bits 2-3 the
 *      filter (0 none, 1 horizontal, 2 vertical, 3 gradient), bits 4-5 pre-processing (0 or 1; 1 is level quantisation,
 *      nothing to undo), bits 6-7 reserved -- then the residuals r.  The inverse filter, sums mod 256, a the alpha:
 *      row 0 of every filter but none a[0][x] = r[0][x] + a[0][x-1] with a[0][0] = r[0][0]; column 0 of the rows below
 *      a[y][0] = r[y][0] + a[y-1][0]; elsewhere horizontal adds a[y][x-1], vertical a[y-1][x], gradient
 *      clip(a[y][x-1] + a[y-1][x] - a[y-1][x-1], 0, 255).
 *      TAKEN: the canonical layout only -- a VP8X chunk of at least 10 bytes with the alpha flag (0x10) set and the
 *      animation flag clear, whose canvas is the `VP8 ` frame's width x height, exactly ONE ALPH chunk in front of the one
 *      `VP8 ` chunk, other chunks skipped (a repeated VP8X among them: the first one's flag and canvas hold).  A VP8X flag with no ALPH chunk gives A = 255, as the lossy route always did.
 *      IMP_ERROR_UNSUPPORTED (the host decoder judges it as before; libwebp's plain decode and its demuxer disagree about
 *      these, and this decoder does not pick a side): an ALPH in front of VP8L, an ALPH behind the image chunk, a second
 *      ALPH, an ALPH without VP8X or with the alpha flag clear, a canvas that differs from the frame, ANIM / ANMF.
 *      IMP_ERROR_DECODE_FAILED: an ALPH chunk of fewer than 2 bytes; a method above 1, pre-processing above 1 or a reserved
 *      bit; a raw plane shorter than w * h; a VP8L stream the lossless decoder fails or that runs past its chunk; and
 *      everything the lossy route fails.  The checks come in one order in all four calls: the container, the frame tag,
 *      the canvas, the header byte, then the frame header and the streams.
 *      HOW: a file with alpha is one lossy item as before.  A raw plane's w * h bytes join the group's ONE upload.  A VP8L
 *      plane is parsed by the lossless front entered without container and header (wd_parse_stream, bit 0 of the byte
 *      behind the header byte) and becomes one more item of the group's three lossless launches: its frame is a scratch
 *      plane of w * h * 4 bytes in the group's device block that never crosses the link, and it has a status word of its
 *      own -- the file fails if either of its two words is set.  Behind k_vp8_dec_frame and k_webp_dec_inverse on the same
 *      stream ONE launch, IMPGPU_WEBP_DEC_ALPHA_LAUNCHES (1) a group that holds an alpha file: k_webp_alpha, a workgroup
 *      a file, reads the raw bytes or byte 1 of each scratch word, undoes the filter and writes byte 3 of every pixel and
 *      nothing else; a file with a status word set is skipped.  None is a copy; horizontal a prefix sum down column 0 and
 *      then one along every row (a wave a row, 64 columns a step); vertical a prefix sum along row 0 and a lane a column
 *      downwards; the gradient, which its clip makes sequential, runs a band of 64 rows in a wave, the rows a column
 *      apart, left / top / top-left moving between lanes in registers and the band's last row to the next band through LDS,
 *      one band after the other (MEASURED below says why not pipelined).  Every loop is bounded by w, h and the band count.
 *      A group launches 3 (lossy) + 1 (alpha), and 3 more when it holds a lossless file or a VP8L plane.  ONE wait per call.
 *      impgpu_webp_alpha_info (host only): info[0] method, [1] filter, [2] pre-processing, [3] the VP8L stream's feature
 *      word as IMPGPU_WEBP_DEC_F_* (0 for a raw plane); IMP_ERROR_UNSUPPORTED for a file with no alpha plane this route
 *      takes, the route's own code for a damaged one.  For a VP8L plane it walks the stream's entropy-coded image (back
 *      references and distance codes show only there) into one buffer of w * h * 4 bytes -- no inverse transform, no
 *      frame; a caller that only routes files needs no more than impgpu_webp_info_ex.
 *      MEASURED (profiles/webp_alpha_decode_probe.json, tools/webp_alpha_decode_probe.py; one session, interleaved, medians after
 *      a warm-up; photo-like colour at quality 75 with (a) a soft mask and (b) a noise alpha, both Pillow-written -- (a) comes
 *      out as a VP8L plane, (b) as a raw one -- and (c) the mask hand-assembled under the gradient filter; the call with accept 3
 *      / the same files' bare `VP8 ` chunks with accept 1 / Pillow's decode on one core + impgpu_image_upload, ms): a lone
 *      640x480 file (a) 117.9 / 105.8 / 2.9, (b) 113.0 / 112.3 / 2.7, (c) 117.2 / 105.6 / 3.5; a lone 1920x1080 file (a) 794 /
 *      717 / 20.0, (b) 772 / 775 / 17.4, (c) 747 / 703 / 24.2; 64 files of 320x240 (a) 35.2 / 28.5 / 52.5, (b) 30.4 / 30.0 / 44.0,
 *      (c) 33.4 / 28.9 / 61.7.  A raw plane costs nothing that shows; a VP8L plane costs 4-12 ms at these sizes and 44-77 ms at
 *      1920x1080, nearly all of it the lossless launches (k_webp_dec_pixels 31-73 ms at 1920x1080 for the mask under the four filters, 84 for Pillow's own file of it), which run in front of the
 *      lossy ones on the one stream.  A lone file still LOSES to the host by 30-40x, as the lossy route does (the one-lane
 *      k_vp8_dec_recon); 64 files of 320x240 a call are ahead 1.4-1.8x.  Per kernel (a separate rocprofv3 --kernel-trace
 *      --stats run, the mask under each filter, k_webp_alpha none / horizontal / vertical / gradient next to
 *      k_vp8_dec_recon, ms): 640x480 0.07 / 0.42 / 0.19 / 1.43 next to 97; 1920x1080 0.67 / 4.13 / 2.16 / 13.6 next to 658;
 *      64 x 320x240 0.03 / 0.16 / 0.12 / 0.63 next to 26.4.  The gradient at 1920x1080 is 2.1 % of that call's k_vp8_dec_recon,
 *      under the tenth that would have called for pipelining its bands across the workgroup's waves: they run one after
 *      the other. ---- */
#define IMPGPU_WEBP_ACCEPT_ALPHA 2
#define IMPGPU_WEBP_DEC_ALPHA_LAUNCHES 1
int impgpu_webp_alpha_info(const unsigned char* blob, size_t size, int info[4]);

/* ---- batch entry points (benchmark / multi-frame albums: bridge.c:578,591,608,632).
 *      `count` frames of identical geometry, frame i at base + i*frame_stride bytes,
 *      already resident in HBM.  stream = hipStream_t to launch on (NULL = env stream).
 *      Asynchronous: returns after enqueue. ---- */
int impgpu_batch_cv_resize(const void* src, long long src_frame_stride, int src_width, int src_height, int src_step,
                           void* dst, long long dst_frame_stride, int dst_width, int dst_height, int dst_step,
                           int channels, int count, int interpolation, void* stream);
/* The per-frame Resize() loop of bridge.c:588-604 over frames that all DIFFER in size (BASELINE configs[4], frames already
 * in HBM): each item is cvResize'd with the interpolation Resize() picks for it -- NN when `simple`, CUBIC when either
 * side grows, AREA otherwise (bridge.c:188-192) -- but frames that share a kernel ride in one launch (a descriptor per
 * frame), so a run of thumbnails costs a handful of launches instead of one per request: one for the general AREA
 * shrinks whose cells span at most 20 source columns (factors up to about 18), one for the shrinks past that
 * with cells of 21..66 columns (factors up to 64: a 4032-wide photo at 200 wide and below, a 600 dpi A4 scan at 150 wide;
 * any channel count, source pointer and pitch -- a BGR crop window may start at any column), one for the AREA shrinks
 * whose two factors are whole numbers, one for the NN frames, one for the BGR / BGRA enlargements (CUBIC with y not
 * shrinking, x shrinking by at most 2 and a source at least 4 columns wide; their coefficient tables travel with the
 * launch and never enter the per-thread table cache; a launch whose tables would pass 4 MB is split) -- at most five
 * per channel count.  In that launch a frame with a whole factor of 2, 3 or 4 runs the generic row loop, not the
 * unrolled form it takes alone.  Timed against one launch per frame: 64 avatars of 64 sizes to 640
 * wide 0.48 -> 0.10 ms, 1024 of them 35 -> 1.2 ms, 64 frames of 480x270 -> 1920x1080 0.58 -> 0.20 ms.  The built
 * tables of an axis are kept in host memory per thread (16 MB at most), so sizes a worker has seen cost a copy.  Gray general AREA
 * shrinks are gathered whatever their source pointer, pitch and destination alignment are: a crop window of a
 * gray scan starts at any byte (launch counts are tested; the gray launch has not yet been timed against the per-frame
 * loop: DESIGN section 4).  A frame that is the only one of its kind in the call, and what no descriptor launch
 * gathers -- gray enlargements, frames of which one axis grows while y shrinks, enlargements whose x shrinks past 2x
 * or whose source is narrower than 4 columns, extreme ratios (cells past 66 source columns, whatever the channel
 * count) -- take one launch each.  Same bytes
 * as calling impgpu_batch_cv_resize once per item.  Nothing is launched if any item is malformed
 * (IMP_ERROR_INVALID_ARGS).  The _ex form also reports the number of kernels it enqueued in *launches (may be NULL). */
typedef struct impgpu_resize_item {
    const void* src; int src_width, src_height, src_step;
    void*       dst; int dst_width, dst_height, dst_step;
} impgpu_resize_item;
int impgpu_batch_resize_mixed(const impgpu_resize_item* items, int count, int channels, int simple, void* stream);
int impgpu_batch_resize_mixed_ex(const impgpu_resize_item* items, int count, int channels, int simple, void* stream,
                                 int* launches);
/* cfg3 chain on a batch: resize (AREA/CUBIC by the reference's rule) -> rotate -> watermark.
 * rotate in {0, 90, 180, 270}; config->watermark may be NULL. dst geometry must match. */
int impgpu_batch_resize_rotate_watermark(const void* src, long long src_frame_stride, int src_width, int src_height, int src_step,
                                         void* dst, long long dst_frame_stride, int dst_step,
                                         int resize_width, int resize_height, int rotate,
                                         const impgpu_config* config, int channels, int count, void* stream);

/* A run of pointwise filter-* requests (everything but flip / rotate / blur) applied in place to every frame of a
 * batch with ONE fused launch: the per-frame filter loop of bridge.c:606-627 for albums (animated GIFs).  Returns
 * IMP_ERROR_UNSUPPORTED if a request is not pointwise (the caller then goes frame by frame), otherwise the code the
 * first failing Filter() would return. */
int impgpu_batch_filters(void* frames, long long frame_stride, int width, int height, int channels, int step, int count,
                         const char* const* filters, int filter_count, int allow_experiments, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMPGPU_H */
