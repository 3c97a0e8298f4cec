// imp_enc_host.h -- the host scaffold the answer encoders share (imp_png_enc.hip, imp_gif_enc.cpp, imp_webp_enc.cpp): a
// group's device block is laid out region by region (BlockLayout) and owned for the call (DevBlock), the records come back
// in a first wait (fetch_records), the fit rule says per answer what it takes and whether it is fetched (answer_fits), and
// the answers that fit come back in a second wait, one pinned area (AnswerFetch).  Host only: include it after
// imp_internal.h; no kernel does.  DESIGN.md section 4h.
#pragma once
#include <cstring>
#include <vector>

namespace imp {

inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

// A device block, carved top to bottom: take() gives the next region's offset and moves on by its size rounded up to 256,
// take_exact() by the size as it is (a term that is a multiple of 256 by construction, or a pool that packs).
struct BlockLayout {
    size_t take(size_t bytes) { return take_exact(up256(bytes)); }
    size_t take_exact(size_t bytes) { const size_t at = end; end += bytes; return at; }
    size_t size() const { return end; }
    size_t end = 0;
};

// v's elements at head[at...): a table of the block's uploaded front
template <class T>
void head_put(std::vector<uint8_t>& head, size_t at, const std::vector<T>& v) {
    if (!v.empty()) std::memcpy(head.data() + at, v.data(), v.size() * sizeof(T));
}

// Pool memory that goes back when the call leaves, by whichever exit.
struct DevBlock {
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete; DevBlock& operator=(const DevBlock&) = delete;
    ~DevBlock() { dev_free(p); }
    uint8_t* bytes() const { return (uint8_t*)p; }
    void* p = nullptr;
};
// The exit for a failure after work was enqueued: what is in flight may still use the block, so the stream drains before the
// owners free (`return drained(rc);`).
inline int drained(int rc) { (void)hipStreamSynchronize(env_stream()); return rc; }

// The first wait: `bytes` at `dev` into `host`, through a pinned buffer held until they are copied out.
inline int fetch_records(const void* dev, size_t bytes, void* host, const char* what) {
    void *pin = nullptr, *token = nullptr;
    if (int rc = stage_begin(bytes, &pin, &token)) return drained(rc);
    const hipError_t e = hipMemcpyAsync(pin, dev, bytes, hipMemcpyDeviceToHost, env_stream());
    if (e != hipSuccess) { set_error(what, e); return drained(IMP_ERROR_DEVICE); }
    stage_hold(token, true);
    const int rc = lane_wait();
    if (!rc) std::memcpy(host, pin, bytes);
    stage_hold(token, false);
    return rc;
}

// The fit rule: *len always says what the answer takes; one longer than its caller's buffer is IMP_ERROR_MALLOC_FAILED
// with nothing written; -> whether to fetch it.  (An answer that outgrew its bound is refused before, at the caller.)
inline bool answer_fits(size_t length, size_t capacity, int* code, size_t* len) {
    *len = length;
    *code = length > capacity ? IMP_ERROR_MALLOC_FAILED : IMP_OK;
    return length <= capacity;
}

// The second wait: every piece add()ed gets a slot of one pinned area (rounded up to 64 bytes); run() enqueues the copies
// and waits, at() is a piece's pinned bytes until the object goes, which releases the area.
class AnswerFetch {
public:
    AnswerFetch() = default;
    AnswerFetch(const AnswerFetch&) = delete; AnswerFetch& operator=(const AnswerFetch&) = delete;
    ~AnswerFetch() { stage_hold(token_, false); }
    int add(const void* dev, size_t bytes) {
        pieces_.push_back(Piece{dev, bytes, total_});
        total_ += (bytes + 63) & ~size_t(63);
        return (int)pieces_.size() - 1;
    }
    int run(const char* what) {
        if (!total_) return IMP_OK;
        void *pin = nullptr, *token = nullptr;
        if (int rc = stage_begin(total_, &pin, &token)) return rc;
        pin_ = (uint8_t*)pin;
        for (const Piece& p : pieces_) {
            const hipError_t e = hipMemcpyAsync(pin_ + p.at, p.dev, p.bytes, hipMemcpyDeviceToHost, env_stream());
            if (e != hipSuccess) { set_error(what, e); return drained(IMP_ERROR_DEVICE); }
        }
        stage_hold(token_ = token, true);
        return lane_wait();
    }
    uint8_t* at(int piece) const { return pin_ + pieces_[(size_t)piece].at; }

private:
    struct Piece { const void* dev; size_t bytes, at; };
    std::vector<Piece> pieces_;
    size_t total_ = 0;
    uint8_t* pin_ = nullptr;
    void* token_ = nullptr;
};

}  // namespace imp
