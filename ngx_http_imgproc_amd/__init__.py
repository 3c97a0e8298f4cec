"""ngx_http_imgproc_amd -- host-side mirror of IMP's operator interface over libimpgpu.so.

The product is the C-ABI library (include/impgpu.h, csrc/); this package is the thin
Python binding the tests and bench.py drive it through.  Names, argument strings and
return codes follow the reference's operators (bridge.h, filters.h): Crop, Resize,
Filter, Watermark, BlendWithPaper, CalcPerceivedBrightness, ASCII, and RunJob's operator
segment.  There is no CPU fallback: importing fails loudly when the library is missing,
and every pixel-touching call fails with IMP_ERROR_DEVICE without a GPU.
"""
from ._lib import lib, LIB_PATH, ImpError  # noqa: F401
from .ops import (  # noqa: F401
    IMP_OK, IMP_ERROR_UNSUPPORTED, IMP_ERROR_MALLOC_FAILED, IMP_ERROR_DECODE_FAILED, IMP_ERROR_INVALID_ARGS, IMP_ERROR_NO_SUCH_FILTER, IMP_ERROR_TOO_BIG_TARGET,
    IMP_ERROR_TOO_MUCH_FILTERS, IMP_ERROR_DEVICE, IMP_ERROR_NO_SUCH_WATERMARK,
    INTER_NN, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4,
    Config, Image, env_start, env_destroy, sync,
    jpeg_info, png_info, png_stage_times, batch_decode_jpeg, batch_decode_jpeg_prepared, batch_decode_png, jpeg_unstuff, jpeg_request_one_wait, batch_encode_jpeg, batch_encode_png, png_deflate, crop_geometry, resize_geometry, filter_check, check_destructive, blur_form,
    JPEG_PROGRESSIVE, batch_decode_jpeg_ex, batch_decode_jpeg_begin_finish_ex, jpeg_info_ex, jpeg_counters,
    PNG_PALETTE, PNG_LOW_GRAY, PNG_ADAM7, PNG_ALL, PNG_DEVICE_INFLATE, png_inflate_lanes, png_info_ex, png_scanlines_ex, batch_decode_png_ex,
    batch_cv_resize, batch_resize_mixed, ResizeItem, batch_resize_rotate_watermark, batch_filters, run_ops, batch_run_ops, Request, gif_compose,
    batch_calc_perceived_brightness, batch_ascii, batch_gif_compose, gif_page_array, batch_download_fi, batch_album_download,
    decode_gif, batch_decode_gif, gif_info, gif_pages, gif_pages_split, GIF_SPLIT, GIF_SPLIT_MIN_BYTES,
    encode_gif, batch_encode_gif, encode_gif_host, gif_encode_bound, GIF_ENC_SEGMENT, gif_quantize_host, GIF_ENC_QUANTIZE, GIF_ENC_DELTA,
    encode_webp, batch_encode_webp, encode_webp_host, webp_encode_bound, WEBP_TILE_BITS, WEBP_ENC_BACKREFS, WEBP_MIN_MATCH,
    decode_webp, batch_decode_webp, webp_decode_host, webp_info, WEBP_ACCEPT_LOSSY, WEBP_DEC_LOSSY_LAUNCHES,
    webp_alpha_info, WEBP_ACCEPT_ALPHA, WEBP_DEC_ALPHA_LAUNCHES,
    encode_webp_lossy, batch_encode_webp_lossy, encode_webp_lossy_host, webp_lossy_encode_bound, request_webp_quality,
)
