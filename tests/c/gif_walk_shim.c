/* impgpu_gif_walk behind one exported symbol: the tests reach the header's static inline walk through this, and the
 * header is compiled as strict C99 on the way (tests/test_gif_decode_host.py). */
#include "impgpu_gif.h"

int gif_walk_shim(const unsigned char* blob, size_t size, impgpu_gif_desc* pages, int cap, int* count, int* canvas_w, int* canvas_h) {
    return impgpu_gif_walk(blob, size, pages, cap, count, canvas_w, canvas_h);
}
