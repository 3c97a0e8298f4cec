// imp_api.cpp -- the operator entry points of include/impgpu.h: each takes the reference's
// argument string, decides everything the reference decides on the CPU before touching pixels
// (imp_args.cpp), then enqueues kernels on the env stream.  impgpu_run_ops is the operator
// segment of RunJob (bridge.c:574-656) with Crop folded into the next operator's source view
// and runs of pointwise filters fused into one launch.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>
#include "imp_internal.h"

using namespace imp;

namespace {

Frames one_frame(const View& v, impgpu_image* dst) {
    Frames f{};
    f.src = v.d; f.src_stride = 0; f.v = v;
    f.dst = dst->d; f.dst_stride = 0; f.dw = dst->w; f.dh = dst->h; f.dstep = dst->step;
    f.count = 1;
    return f;
}

// The image -- or album -- being worked on: `owner` holds the memory, `v` is the window of its frame 0 that is the
// current frame (smaller than owner after a folded Crop); frame i of an album is the same window `stride()` bytes on.
struct Work {
    impgpu_image* owner;
    View v;
    int count() const { return owner->frames; }
    long long stride() const { return (long long)owner->fstride; }
    bool is_view() const { return v.d != owner->d || v.w != owner->w || v.h != owner->h; }
    void adopt(impgpu_image* im) {
        image_delete(owner);
        owner = im;
        v = view_of(im);
    }
    // a fresh destination with this work's frame count
    int fresh(int w, int h, int c, impgpu_image** out) const { return image_new_album(w, h, c, owner->frames, out); }
    Frames to(impgpu_image* dst) const {
        Frames f = one_frame(v, dst);
        f.src_stride = stride(); f.dst_stride = (long long)dst->fstride; f.count = owner->frames;
        return f;
    }
    uint8_t* px() const { return const_cast<uint8_t*>(v.d); }
};

int materialize(Work& wk) {
    if (!wk.is_view()) return IMP_OK;
    impgpu_image* out = nullptr;
    if (int rc = wk.fresh(wk.v.w, wk.v.h, wk.v.c, &out)) return rc;
    if (int rc = launch_copy(wk.to(out), env_stream())) { image_delete(out); return rc; }
    wk.adopt(out);
    return IMP_OK;
}

int do_resize(Work& wk, int w, int h, int interp) {
    impgpu_image* out = nullptr;
    if (int rc = wk.fresh(w, h, wk.v.c, &out)) return rc;
    if (int rc = launch_cv_resize(wk.to(out), interp, env_stream())) { image_delete(out); return rc; }
    wk.adopt(out);
    return IMP_OK;
}

int flush_program(Work& wk, PixelProgram& prog) {
    if (prog.empty()) return IMP_OK;
    int rc = launch_pixel_program(wk.px(), wk.stride(), wk.v.w, wk.v.h, wk.v.c, wk.v.step, wk.count(), prog, env_stream());
    prog.clear();
    return rc;
}

int apply_plan(Work& wk, const FilterPlan& plan) {
    switch (plan.cls) {
        case FC_FLIP: {
            impgpu_image* out = nullptr;
            if (int rc = wk.fresh(wk.v.w, wk.v.h, wk.v.c, &out)) return rc;
            if (int rc = launch_flip(wk.to(out), plan.flip_mode, env_stream())) { image_delete(out); return rc; }
            wk.adopt(out);
            return IMP_OK;
        }
        case FC_ROTATE: {
            impgpu_image* out = nullptr;
            const bool swap = plan.rotate != 180;
            if (int rc = wk.fresh(swap ? wk.v.h : wk.v.w, swap ? wk.v.w : wk.v.h, wk.v.c, &out)) return rc;
            if (int rc = launch_rotate(wk.to(out), plan.rotate, env_stream())) { image_delete(out); return rc; }
            wk.adopt(out);
            return IMP_OK;
        }
        case FC_BLUR: {
            if (wk.v.c == 4 || wk.v.c == 3) {      // one-pass fused kernel into a fresh frame; falls through when it does not apply
                impgpu_image* out = nullptr;
                if (int rc = wk.fresh(wk.v.w, wk.v.h, wk.v.c, &out)) return rc;
                int rc = launch_gaussian_fused(wk.to(out), plan.sigma, env_stream());
                if (rc == IMP_OK) { wk.adopt(out); return IMP_OK; }
                image_delete(out);
                if (rc != IMP_ERROR_UNSUPPORTED) return rc;
            }
            return launch_gaussian(wk.px(), wk.stride(), wk.v.w, wk.v.h, wk.v.c, wk.v.step, wk.count(), plan.sigma, env_stream());
        }
        default:
            return IMP_OK;
    }
}

int do_filter(Work& wk, const char* request, int allow, PixelProgram& prog) {
    FilterPlan plan;
    if (int rc = filter_plan(request, allow, wk.v.c, wk.v.w, wk.v.h, &plan, &prog)) return rc;
    if (plan.cls == FC_POINTWISE || plan.cls == FC_NOOP) return IMP_OK;     // stays queued in prog
    if (int rc = flush_program(wk, prog)) return rc;
    return apply_plan(wk, plan);
}

// The overlay of `cfg` on a frame of w x h, as every launch that blends it takes it: the rectangle (watermark_rect), the
// overlay's pixels, and alpha = 1 - opacity / 100 (bridge.c:275, filters.c:620).  cfg->watermark must be set.
int overlay_args(const impgpu_config* cfg, int w, int h, OverlayArgs* a) {
    const impgpu_image* ov = cfg->watermark;
    if (int rc = watermark_rect(w, h, ov->w, ov->h, cfg, &a->rx, &a->ry, &a->maxcol, &a->maxrow)) return rc;
    a->ov = ov->d; a->ostep = ov->step;
    a->alpha = 1 - (float)(cfg->watermark_opacity / 100.0);
    return IMP_OK;
}

bool bgra_overlay(const impgpu_image* ov) {                           // what the resize tail's overlay path takes
    return ov && ov->c == 4 && !(((uintptr_t)ov->d | (uintptr_t)ov->step) & 3);
}

int do_watermark(Work& wk, const impgpu_config* cfg) {
    if (wk.v.c < 3 || cfg->watermark->c < 3) return IMP_ERROR_INVALID_ARGS;   // reference indexes B,G,R unconditionally
    OverlayArgs a{};
    if (int rc = overlay_args(cfg, wk.v.w, wk.v.h, &a)) return rc;
    return launch_blend_over(wk.px(), wk.stride(), wk.v.w, wk.v.h, wk.v.c, wk.v.step, wk.count(), cfg->watermark,
                             a.rx, a.ry, a.maxcol, a.maxrow, a.alpha, env_stream());
}

// Does the row-streaming AREA kernel with a tail on its stores (area_tail_plan) take the resize of `count` frames at `v` to
// w x h, the frame turned by `rot` as it is stored?
bool area_tail_takes(const View& v, int count, int w, int h, int rot) {
    const bool swap = rot == 90 || rot == 270;
    Frames f{};
    f.src = v.d; f.v = v; f.dw = w; f.dh = h; f.dstep = aligned_step(swap ? h : w, v.c); f.count = count;
    int ww, bh;
    return area_tail_plan(f, &ww, &bh);
}

// The fused-turn rule, stated once for impgpu_run_ops and chain_plan, which must agree on it: the first filter of a colour
// request rides the stores of its INTER_AREA resize to w x h when it is a turn and area_tail_plan takes that resize; the
// overlay rides along (the watermark step is then done) when the turn is the only filter and the overlay is BGRA.  Returns
// the turn, 0 when nothing rides.  Whether the overlay's rectangle can be computed is the caller's to ask (overlay_args).
int fused_turn(const View& v, int count, int w, int h, int interp, const impgpu_job* job, const impgpu_config* cfg, bool* with_wm) {
    *with_wm = false;
    if (interp != IMP_INTER_AREA || (v.c != 4 && v.c != 3) || job->filter_count < 1) return 0;    // BGRA, and BGR: every JPEG
    FilterPlan first;
    PixelProgram none;
    if (filter_plan(job->filters[0], cfg->allow_experiments, v.c, w, h, &first, &none) != IMP_OK || first.cls != FC_ROTATE) return 0;
    if (!area_tail_takes(v, count, w, h, first.rotate)) return 0;
    *with_wm = job->filter_count == 1 && bgra_overlay(cfg->watermark);
    return first.rotate;
}

// What impgpu_batch_run_ops needs to know to run a request in shared launches instead of through impgpu_run_ops: a single
// colour or gray frame, or a colour album (planned ONCE: crop, resize geometry, filter plans and overlay placement are the
// same for all its frames; every frame then is an item of its own), whose chain is [crop ->] [resize ->] any filters ->
// [watermark] -> [flatten], every decision made here on the host.  Host-only, no fault point entered: a request this refuses goes to impgpu_run_ops whole.
// Without a resize (`sized` false) nothing rides a resize launch -- rot, wm_turn and the folds stay clear -- and the chain is
// the segment list alone, its first segment reading the window `v`.
// The resize is launch_resize_mixed, or the row-streaming AREA kernel with a tail on its stores (k_resize_area_mix_tail,
// the one acceptance test area_tail_plan) when something rides there: the first filter when it is a turn, as impgpu_run_ops
// fuses it (with the overlay when the turn is the only filter and the overlay is BGRA, as that launch carries it too), and
// -- when nothing but the watermark and the flatten follows the resize -- the tail.  The rest of the chain is a list of
// segments, each one launch of its own kind: a pointwise run (do_filter's PixelProgram, cut where launch_pixel_program cuts
// it), a barrier (one blur, flip or turn), and the tail -- the last run, the watermark and the flatten as one per-pixel pass.
enum SegKind { SEG_PIXEL = 0, SEG_BLUR, SEG_GEOM };
struct Segment {
    int kind;
    int step;                   // what a failure of its launch reports
    PixelProgram prog;          // SEG_PIXEL
    bool has_wm, flat;          // SEG_PIXEL: the tail's watermark / flatten
    FilterPlan plan;            // SEG_BLUR / SEG_GEOM
    int w, h;                   // the frame entering the segment
};
struct ChainPlan {
    View v;                     // the source window (after the crop)
    int w, h, interp;           // the resize
    int fw, fh;                 // the frame the resize launch leaves (turned when rot is 90 / 270)
    int rot;                    // first filter turned on the AREA stores (0: none)
    bool wm_turn;               // the overlay rides the turn's launch, as in impgpu_run_ops: part of the resize step
    bool fold_wm, fold_flat;    // the tail (watermark, flatten) folded onto the resize's stores
    std::vector<Segment> segs;
    OverlayArgs wm;             // the overlay's placement on the final frame
    bool gray;                  // a gray frame: resized as gray, promoted (bridge.c:613-618), then a BGR frame's segments
    bool sized;                 // the request has a resize
};

bool chain_plan(const impgpu_image* im, const impgpu_job* job, const impgpu_config* cfg, ChainPlan* p) {
    if (!im || !job || !cfg || im->frames < 1 || (im->c != 1 && im->c != 3 && im->c != 4) || job->filter_count < 0) return false;
    if (im->c == 1 && im->frames != 1) return false;                   // gray albums: impgpu_run_ops (composes and FreeImage frames are BGRA)
    if (cfg->max_filters_count > 0 && job->filter_count > cfg->max_filters_count) return false;
    if (job->filter_count > 0 && !job->filters) return false;
    for (int i = 0; i < job->filter_count; i++) if (!job->filters[i]) return false;
    View v = view_of(im);
    if (job->crop) {
        int x, y, w, h;
        if (crop_geometry(v.w, v.h, job->crop, job->gravity, &x, &y, &w, &h) != IMP_OK) return false;
        v = view_sub(v, x, y, w, h);
    }
    const bool sized = job->resize != nullptr;
    int w = v.w, h = v.h, interp = IMP_INTER_AREA;
    if (sized && resize_geometry(v.w, v.h, job->resize, cfg->max_target_w, cfg->max_target_h, job->simple, &w, &h, &interp) != IMP_OK) return false;
    // a gray frame is BGR from the filtering step on (impgpu_run_ops promotes it there): its filters and its overlay are
    // planned for 3 channels, and nothing rides its resize -- fused_turn and area_tail_plan take colour frames only
    const bool gray = v.c == 1;
    const int c = gray ? 3 : v.c;
    const impgpu_image* ov = cfg->watermark;
    p->gray = gray;
    p->sized = sized;
    p->v = v; p->w = w; p->h = h; p->interp = interp;
    p->wm_turn = p->fold_wm = p->fold_flat = false;
    p->wm = OverlayArgs{};
    p->segs.clear();
    p->rot = sized ? fused_turn(v, 1, w, h, interp, job, cfg, &p->wm_turn) : 0;        // (count 1: every frame is an item of its own)
    const bool swap = p->rot == 90 || p->rot == 270;
    int cw = swap ? h : w, ch = swap ? w : h;
    const int i0 = p->rot ? 1 : 0;
    p->fw = cw; p->fh = ch;
    auto push_runs = [&](const PixelProgram& prog, PixelProgram* tail) {
        std::vector<PixelProgram> parts;
        if (!prog.empty()) split_program(prog, &parts);
        for (size_t k = 0; k < parts.size(); k++) {
            if (tail && k + 1 == parts.size()) { *tail = parts[k]; break; }
            Segment sg{};
            sg.kind = SEG_PIXEL; sg.step = IMP_STEP_FILTERING; sg.prog = parts[k]; sg.w = cw; sg.h = ch;
            p->segs.push_back(sg);
        }
    };
    PixelProgram prog;
    for (int i = i0; i < job->filter_count; i++) {                     // do_filter, planned
        FilterPlan plan;
        if (filter_plan(job->filters[i], cfg->allow_experiments, c, cw, ch, &plan, &prog) != IMP_OK) return false;
        if (plan.cls == FC_POINTWISE || plan.cls == FC_NOOP) continue;
        push_runs(prog, nullptr);
        prog.clear();
        Segment sg{};
        sg.kind = plan.cls == FC_BLUR ? SEG_BLUR : SEG_GEOM;
        sg.step = IMP_STEP_FILTERING; sg.plan = plan; sg.w = cw; sg.h = ch;
        p->segs.push_back(sg);
        if (plan.cls == FC_ROTATE && plan.rotate != 180) std::swap(cw, ch);
    }
    Segment tail{};
    tail.kind = SEG_PIXEL; tail.w = cw; tail.h = ch;
    push_runs(prog, &tail.prog);
    if (ov) {                                                          // do_watermark, planned
        if (c < 3 || ov->c < 3) return false;
        // (impgpu_run_ops goes on without the fused overlay and fails at its watermark step: refused, so that it takes that route)
        if (overlay_args(cfg, cw, ch, &p->wm) != IMP_OK) return false;
        tail.has_wm = !p->wm_turn;                                     // (on the turn's launch: the watermark step is done there)
    }
    tail.flat = job->need_flatten && c == 4;
    // nothing but the watermark and the flatten after the resize: they ride the resize's stores
    if (p->segs.empty() && tail.prog.empty() && (tail.has_wm || tail.flat) && (!tail.has_wm || bgra_overlay(ov)) &&
        (p->rot != 0 || (sized && interp == IMP_INTER_AREA && area_tail_takes(v, 1, w, h, 0)))) {
        p->fold_wm = tail.has_wm;
        p->fold_flat = tail.flat;
        return true;
    }
    tail.step = tail.prog.empty() ? IMP_STEP_WATERMARK : IMP_STEP_FILTERING;
    if (!tail.prog.empty() || tail.has_wm || tail.flat) p->segs.push_back(tail);
    return true;
}

// ------------------------------------------------------------------ impgpu_batch_run_ops: requests in shared launches
// The items of one launch and the requests they belong to.
template <class Item> struct Group {
    std::vector<Item> items;
    std::vector<int> who;
    void add(int i, Item it) { items.push_back(it); who.push_back(i); }
    bool empty() const { return items.empty(); }
    int size() const { return (int)items.size(); }
};

// One request of the call.
struct ChainRun {
    ChainPlan plan;
    View cur{};                      // the frame it stands on: a window of images[i] until something writes a fresh frame (without
                                     // a resize it starts on its crop window, as impgpu_run_ops' Work does), then the whole of it
    impgpu_image* pending = nullptr; // the fresh frame of its launch in flight
    int nsegs = 0;                   // segments it runs (fewer than the plan's when a fault point cut it)
    int code = IMP_OK, step = IMP_STEP_INFO;   // the verdict it reports if every launch of its succeeds
    int at = IMP_STEP_START;         // the step it is working on: what a failed allocation or launch of its reports
    // LONE: answered by impgpu_run_ops.  WAITING: its resize has not landed.  RUNNING: in the rounds, its verdict published.
    // STOPPED: a fault point before its first launch, an allocation or a launch failed it; codes[i] / steps[i] say so.
    enum { LONE, WAITING, RUNNING, STOPPED } state = LONE;
    bool cut = false;                // a fault point fired behind the resize: impgpu_run_ops' `done:` exit, which never
                                     // materializes and whose pointwise runs have worked in place on the window
};

struct Batch {
    impgpu_image** images; const impgpu_job* jobs; const impgpu_config* const* configs; int count; int* codes; int* steps;
    hipStream_t s;
    std::vector<ChainRun> runs;
    // round 0, per channel slot (c - 3; gray: 2, which has no tails): requests with something on the resize's stores ->
    // k_resize_area_mix_tail, bare resizes -> launch_resize_mixed, NN resizes of `simple` requests -> one of their own
    Group<TailItem> tails[2];
    Group<MixFrame> bares[3], nns[3];
    std::vector<int> promote;        // gray requests that reach the promotion
    size_t rounds = 0;               // the longest chain
    // An album that is the only colour album of its call stays with impgpu_run_ops, whose launches are one per operator over
    // all its frames already (the rule of the lone blur forms: sharing is for what comes in numbers).
    bool share_albums = false;
    int album_frames = 0;            // frames of albums admitted to the shared launches so far (at most MAX_ALBUM_FRAMES)
    static constexpr int MAX_ALBUM_FRAMES = 4096;

    // Frame f of request i as its launches see it: `src` bytes on from the frame it stands on (run.cur, a window of frame 0
    // of images[i]), `dst` bytes on from frame 0 of `out` (nullptr: in place).  A single image is an album of one.
    template <class F> void each_frame(int i, const impgpu_image* out, F item) const {
        const impgpu_image* im = images[i];
        for (int f = 0; f < im->frames; f++) item((size_t)f * im->fstride, out ? (size_t)f * out->fstride : (size_t)f * im->fstride);
    }

    bool on_window(int i) const {
        const View& v = runs[(size_t)i].cur;
        return v.d != images[i]->d || v.w != images[i]->w || v.h != images[i]->h;
    }
    void stop(int i, int rc) {
        codes[i] = rc;
        steps[i] = runs[(size_t)i].at;
        runs[(size_t)i].state = ChainRun::STOPPED;
    }
    void publish(int i) {
        codes[i] = runs[(size_t)i].code;
        steps[i] = runs[(size_t)i].step;
        runs[(size_t)i].state = ChainRun::RUNNING;
    }
    // the destination of request i's next launch (as Work::fresh); failed, the request stops with the allocator's code
    impgpu_image* fresh(int i, int w, int h, int c) {
        if (int rc = image_new_album(w, h, c, images[i]->frames, &runs[(size_t)i].pending)) { stop(i, rc); return nullptr; }
        return runs[(size_t)i].pending;
    }
    // A launch is done.  Its fresh frames replace the old ones (pool memory: recycled in stream order, behind the launch); failed,
    // every request of it keeps the frame it had and stops with IMP_ERROR_DEVICE at its step.  `landed`: the launch was the
    // request's resize -- it joins the rounds and its verdict is published.  (An in-place launch has no fresh frames.)
    // Once per request: an album's frames are items of their own, next to each other in `who`.
    void adopt(const std::vector<int>& who, int rc, bool landed = false) {
        for (size_t k = 0; k < who.size(); k++) {
            const int i = who[k];
            if (k > 0 && who[k - 1] == i) continue;
            ChainRun& run = runs[(size_t)i];
            impgpu_image* out = run.pending;
            run.pending = nullptr;
            if (rc != IMP_OK) { image_delete(out); stop(i, IMP_ERROR_DEVICE); continue; }
            if (out) {
                image_delete(images[i]);
                images[i] = out;
                run.cur = view_of(out);
            }
            if (landed) publish(i);
        }
    }
    void admit(int i);
    void resize_round();
    void promote_gray();
    void segment_round(size_t r);
};

// The contract with impgpu_run_ops, for every kind of request.  Fault points: request i enters its own before request i + 1
// does, in impgpu_run_ops' order (bridge.c:574-640) and before any shared launch of the call -- CROP with a crop, RESIZE
// with a resize, FILTERING with filters or a gray frame (its promotion belongs to that step), WATERMARK with an overlay; a
// request the planner refuses is answered by impgpu_run_ops right here, so that its points fall between its neighbours'.
// The frame a request keeps: cut at CROP or RESIZE it keeps its own, untouched.  Cut behind the resize it runs what
// impgpu_run_ops has run by then: at FILTERING the resized frame (with what rides that launch: the turn, and the overlay of
// a lone turn) or, without a resize, its uncropped frame, a gray one unpromoted; at WATERMARK the filtered one, never
// overlaid after the filters, never flattened -- and never copied out of its window.  A failed allocation reports the
// allocator's code, a failed launch IMP_ERROR_DEVICE, both at the step the launch belongs to (ChainRun::at: the resize
// step, FILTERING for the promotion, the segment's own step, WATERMARK for the copy out of the window behind the last
// segment, as impgpu_run_ops' materialize); the request keeps the frame it stood on.  An album is ONE request in all of
// this: its points are entered once per step, never per frame, and what it keeps is the whole album.
void Batch::admit(int i) {
    const impgpu_job* job = &jobs[i];
    const impgpu_config* cfg = configs[i];
    ChainRun& run = runs[(size_t)i];
    ChainPlan& cp = run.plan;
    // (an album past the call's frame bound is answered like a request the planner refuses: right here, in request order)
    const int nframes = images[i] ? images[i]->frames : 1;
    if ((nframes > 1 && (!share_albums || album_frames + nframes > MAX_ALBUM_FRAMES)) || !chain_plan(images[i], job, cfg, &cp)) {
        codes[i] = impgpu_run_ops(&images[i], job, cfg, &steps[i]);
        return;
    }
    if (nframes > 1) album_frames += nframes;
    run.at = IMP_STEP_CROP;
    if (job->crop && fault_hit(IMP_STEP_CROP)) return stop(i, IMP_ERROR_DEVICE);
    if (cp.sized) {
        run.at = IMP_STEP_RESIZE;
        if (fault_hit(IMP_STEP_RESIZE)) return stop(i, IMP_ERROR_DEVICE);
    }
    int failed = -1;
    if ((cp.gray || job->filter_count > 0) && fault_hit(IMP_STEP_FILTERING)) failed = IMP_STEP_FILTERING;
    else if (cfg->watermark && fault_hit(IMP_STEP_WATERMARK)) failed = IMP_STEP_WATERMARK;
    run.nsegs = (int)cp.segs.size();
    if (failed >= 0) {                                              // trim the plan to what impgpu_run_ops has run by then
        run.code = IMP_ERROR_DEVICE;
        run.step = failed;
        run.cut = true;
        cp.fold_wm = cp.fold_flat = false;
        if (failed == IMP_STEP_FILTERING) run.nsegs = 0;
        else if (run.nsegs > 0 && cp.segs.back().kind == SEG_PIXEL && (cp.segs.back().has_wm || cp.segs.back().flat)) {
            Segment& t = cp.segs.back();
            t.has_wm = t.flat = false;
            if (t.prog.empty()) run.nsegs--;
        }
    }
    rounds = std::max(rounds, (size_t)run.nsegs);
    if (cp.gray && failed != IMP_STEP_FILTERING) promote.push_back(i);
    if (!cp.sized) {                                                // no resize launch to wait for: it starts on its window
        run.cur = cp.v;
        return publish(i);
    }
    impgpu_image* out = fresh(i, cp.fw, cp.fh, cp.v.c);
    if (!out) return;
    run.state = ChainRun::WAITING;
    const int k = cp.gray ? 2 : cp.v.c - 3;
    const bool on_stores = cp.wm_turn || cp.fold_wm;
    each_frame(i, out, [&](size_t so, size_t dn) {
        View v = cp.v;
        v.d += so;
        if (cp.rot || on_stores || cp.fold_flat)
            tails[k].add(i, TailItem{v, out->d + dn, cp.w, cp.h, out->step, cp.rot, on_stores, on_stores ? cp.wm : OverlayArgs{}, cp.fold_flat});
        else
            (job->simple ? nns : bares)[k].add(i, MixFrame{v.d, v.w, v.h, v.step, out->d + dn, cp.w, cp.h, out->step});
    });
}

// Round 0: every resize, per slot bare, NN, tail.  A request whose launch fails keeps its frame and stops there.
void Batch::resize_round() {
    static const int slot_cn[3] = {3, 4, 1};
    for (int k = 0; k < 3; k++) {
        if (!bares[k].empty()) adopt(bares[k].who, launch_resize_mixed(bares[k].items.data(), bares[k].size(), slot_cn[k], 0, s), true);
        if (!nns[k].empty()) adopt(nns[k].who, launch_resize_mixed(nns[k].items.data(), nns[k].size(), slot_cn[k], 1, s), true);
        if (k < 2 && !tails[k].empty()) adopt(tails[k].who, launch_area_tail_mixed(tails[k].items.data(), tails[k].size(), k + 3, s), true);
    }
}

// The promotion of every gray request whose resize went through, or that has none and is promoted from its window
// (bridge.c:613-618), ONE launch into fresh BGR frames.  From here on the frames are BGR requests' frames.
void Batch::promote_gray() {
    Group<Gray2BgrItem> g2b;
    for (int i : promote) {
        ChainRun& run = runs[(size_t)i];
        if (run.state != ChainRun::RUNNING) continue;               // (its resize failed)
        run.at = IMP_STEP_FILTERING;
        const View cur = run.cur;
        if (impgpu_image* out = fresh(i, cur.w, cur.h, 3)) g2b.add(i, Gray2BgrItem{cur.d, out->d, cur.w, cur.h, cur.step, out->step});
    }
    if (!g2b.empty()) adopt(g2b.who, launch_gray2bgr_mixed(g2b.items.data(), g2b.size(), s));
}

// Round r: segment r of every chain that has one, one launch per (kind, channel count) in the order window, pixel, geom, blur
// -- and the blur forms no mixed kernel takes one request at a time, as apply_plan runs them (an album: one launch or launch
// pair over all its frames); so does a two-pass blur that is the only REQUEST of its channel and plane count in the round (a
// shared launch pair would save it nothing).  Every frame of an album is an item of its own in its request's group.
// Barriers write fresh frames; pointwise segments work in place, or out of the window into a fresh frame when the request still stands on one.  A request
// that has run its segments and still stands on a window (no segment at all: the bare crop; or nothing but blurs that worked in
// place) leaves it as materialize() does, as a bare item of the window launch of the round after its last segment.
void Batch::segment_round(size_t r) {
    Group<WindowItem> wnd[2];
    Group<PixelTailItem> pix[2];
    Group<GeomItem> geo[2];
    Group<BlurItem> blu[2];
    std::vector<int> pairs[2][2];                                   // two-pass blurs by channel count and plane count (2, 3)
    auto lone_blur = [&](int i, const Segment& sg) {                // a blur form of its own: launched alone, as apply_plan does
        Work wk{images[i], runs[(size_t)i].cur};
        const int rc = apply_plan(wk, sg.plan);
        images[i] = wk.owner;
        runs[(size_t)i].cur = wk.v;
        if (rc) stop(i, rc);
    };
    for (int i = 0; i < count; i++) {
        ChainRun& run = runs[(size_t)i];
        if (run.state != ChainRun::RUNNING || (size_t)run.nsegs < r) continue;
        const View cur = run.cur;
        const int k = cur.c - 3;
        if ((size_t)run.nsegs == r) {                               // behind its last segment: out of the window
            if (run.cut || cur.c < 3 || !on_window(i)) continue;
            run.at = IMP_STEP_WATERMARK;
            impgpu_image* out = fresh(i, cur.w, cur.h, cur.c);
            if (!out) continue;
            each_frame(i, out, [&](size_t so, size_t dn) {
                WindowItem it{};
                it.src = cur.d + so; it.sstep = cur.step;
                it.t.d = out->d + dn; it.t.w = out->w; it.t.h = out->h; it.t.step = out->step;
                wnd[k].add(i, it);
            });
            continue;
        }
        const Segment& sg = run.plan.segs[r];
        run.at = sg.step;
        if (sg.kind == SEG_PIXEL) {
            PixelTailItem it{};
            it.d = const_cast<uint8_t*>(cur.d); it.w = cur.w; it.h = cur.h; it.step = cur.step; it.prog = &sg.prog;
            if (sg.has_wm) {
                const OverlayArgs& wm = run.plan.wm;
                it.has_wm = true; it.ov = configs[i]->watermark;
                it.rx = wm.rx; it.ry = wm.ry; it.maxcol = wm.maxcol; it.maxrow = wm.maxrow; it.alpha = wm.alpha;
            }
            it.flatten = sg.flat;
            if (!on_window(i) || run.cut) {                          // in place (on the window when a fault point cut the request)
                each_frame(i, nullptr, [&](size_t so, size_t) {
                    PixelTailItem at = it;
                    at.d += so;
                    pix[k].add(i, at);
                });
                continue;
            }
            impgpu_image* out = fresh(i, cur.w, cur.h, cur.c);       // out of the window into a fresh frame
            if (!out) continue;
            it.step = out->step;
            each_frame(i, out, [&](size_t so, size_t dn) {
                PixelTailItem at = it;
                at.d = out->d + dn;
                wnd[k].add(i, WindowItem{cur.d + so, cur.step, at});
            });
            continue;
        }
        if (sg.kind == SEG_BLUR) {
            int planes = 0;
            const int form = blur_form(cur.w, cur.h, cur.c, !(((uintptr_t)cur.d | (uintptr_t)cur.step) & 3), sg.plan.sigma, &planes);
            if (form == BLUR_LONE) { lone_blur(i, sg); continue; }
            if (form == BLUR_MIXABLE_PAIR) { pairs[k][planes - 2].push_back(i); continue; }     // (placed behind the loop)
        }
        const bool turn = sg.kind == SEG_GEOM && sg.plan.cls == FC_ROTATE, swap = turn && sg.plan.rotate != 180;
        impgpu_image* out = fresh(i, swap ? cur.h : cur.w, swap ? cur.w : cur.h, cur.c);
        if (!out) continue;
        each_frame(i, out, [&](size_t so, size_t dn) {
            if (sg.kind == SEG_GEOM)
                geo[k].add(i, GeomItem{cur.d + so, cur.w, cur.h, cur.step, out->d + dn, out->w, out->h, out->step, turn ? 1 : 0,
                                       turn ? sg.plan.rotate : sg.plan.flip_mode});
            else
                blu[k].add(i, BlurItem{cur.d + so, out->d + dn, cur.w, cur.h, cur.step, out->step, (double)sg.plan.sigma});
        });
    }
    for (int k = 0; k < 2; k++)
        for (const std::vector<int>& cls : pairs[k])
            for (int i : cls) {
                const Segment& sg = runs[(size_t)i].plan.segs[r];
                if (cls.size() == 1) { lone_blur(i, sg); continue; }
                const View cur = runs[(size_t)i].cur;
                if (impgpu_image* out = fresh(i, cur.w, cur.h, cur.c))
                    each_frame(i, out, [&](size_t so, size_t dn) {
                        blu[k].add(i, BlurItem{cur.d + so, out->d + dn, cur.w, cur.h, cur.step, out->step, (double)sg.plan.sigma});
                    });
            }
    for (int k = 0; k < 2; k++) {
        if (!wnd[k].empty()) adopt(wnd[k].who, launch_window_mixed(wnd[k].items.data(), wnd[k].size(), k + 3, s));
        if (!pix[k].empty()) adopt(pix[k].who, launch_pixel_tail_mixed(pix[k].items.data(), pix[k].size(), k + 3, s));
        if (!geo[k].empty()) adopt(geo[k].who, launch_geom_mixed(geo[k].items.data(), geo[k].size(), k + 3, s));
        if (!blu[k].empty()) adopt(blu[k].who, launch_blur_mixed(blu[k].items.data(), blu[k].size(), k + 3, s));
    }
}

}  // namespace

extern "C" {

int impgpu_crop_geometry(int width, int height, const char* args, const char* gravity, int* x, int* y, int* w, int* h) {
    if (!args || !x || !y || !w || !h) return IMP_ERROR_INVALID_ARGS;
    return crop_geometry(width, height, args, gravity, x, y, w, h);
}

int impgpu_resize_geometry(int width, int height, const char* args, const impgpu_config* config, int simple,
                           int* w, int* h, int* interpolation) {
    if (!args || !w || !h || !interpolation) return IMP_ERROR_INVALID_ARGS;
    return resize_geometry(width, height, args, config ? config->max_target_w : 0, config ? config->max_target_h : 0,
                           simple, w, h, interpolation);
}

int impgpu_filter_check(const char* request, int allow_experiments) {
    if (!request) return IMP_ERROR_INVALID_ARGS;
    FilterPlan plan;
    PixelProgram prog;
    return filter_plan(request, allow_experiments, 4, 64, 64, &plan, &prog);
}

int impgpu_check_destructive(const char* request) { return check_destructive(request); }

int impgpu_blur_form(int width, int height, int channels, double sigma, int* planes) {
    int kernel = 0;
    blur_form(width, height, channels, true, sigma, planes, &kernel);
    return kernel;
}

int impgpu_image_clone(const impgpu_image* src, impgpu_image** out) {
    if (!src || !out) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    impgpu_image* im = nullptr;
    Work wk{const_cast<impgpu_image*>(src), view_of(src)};
    if (int rc = wk.fresh(src->w, src->h, src->c, &im)) return rc;
    if (int rc = launch_copy(wk.to(im), env_stream())) { image_delete(im); return rc; }
    *out = im;
    return IMP_OK;
}

int impgpu_crop(impgpu_image** pointer, const char* args, const char* gravity) {
    if (!pointer || !*pointer || !args) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    int x, y, w, h;
    if (int rc = crop_geometry((*pointer)->w, (*pointer)->h, args, gravity, &x, &y, &w, &h)) return rc;
    Work wk{*pointer, view_sub(view_of(*pointer), x, y, w, h)};
    int rc = IMP_OK;
    if (wk.is_view()) rc = materialize(wk);
    else {   // full-frame crop still yields a fresh image in the reference; the pixels are identical
    }
    *pointer = wk.owner;
    return rc;
}

int impgpu_resize(impgpu_image** pointer, const char* args, const impgpu_config* config, int simple) {
    if (!pointer || !*pointer || !args) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    int w, h, interp;
    if (int rc = resize_geometry((*pointer)->w, (*pointer)->h, args, config ? config->max_target_w : 0,
                                 config ? config->max_target_h : 0, simple, &w, &h, &interp))
        return rc;
    Work wk{*pointer, view_of(*pointer)};
    int rc = do_resize(wk, w, h, interp);
    *pointer = wk.owner;
    return rc;
}

int impgpu_cv_resize(impgpu_image** pointer, int width, int height, int interpolation) {
    if (!pointer || !*pointer || width <= 0 || height <= 0) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    Work wk{*pointer, view_of(*pointer)};
    int rc = do_resize(wk, width, height, interpolation);
    *pointer = wk.owner;
    return rc;
}

int impgpu_filter(impgpu_image** pointer, const char* request, int allow_experiments) {
    if (!pointer || !*pointer || !request) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    Work wk{*pointer, view_of(*pointer)};
    PixelProgram prog;
    int rc = do_filter(wk, request, allow_experiments, prog);
    if (!rc) rc = flush_program(wk, prog);
    *pointer = wk.owner;
    return rc;
}

int impgpu_prepare_watermark(impgpu_config* config, const unsigned char* pixels, int width, int height,
                             int channels, int step) {
    if (!config || !pixels) return IMP_ERROR_NO_SUCH_WATERMARK;
    if (int rc = need_env()) return rc;
    impgpu_image* im = nullptr;
    if (int rc = impgpu_image_upload(pixels, width, height, channels, step, &im)) return rc == IMP_ERROR_INVALID_ARGS ? IMP_ERROR_NO_SUCH_WATERMARK : rc;
    if (config->watermark) image_delete(config->watermark);
    config->watermark = im;
    return impgpu_sync();   // the overlay is read by every lane's stream afterwards: make the upload complete now
}

int impgpu_watermark(impgpu_image* image, const impgpu_config* config) {
    if (!image || !config || !config->watermark) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    Work wk{image, view_of(image)};
    return do_watermark(wk, config);
}

int impgpu_blend_with_paper(impgpu_image* image) {
    if (!image) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    if (image->c != 4) return IMP_ERROR_INVALID_ARGS;   // reference reads channel 3 unconditionally; RunJob only calls it for 4 channels
    return launch_blend_paper(image->d, (long long)image->fstride, image->w, image->h, image->step, image->frames, env_stream());
}

// impgpu_image_download_fi for every frame of an album: each frame's flip and repack into one device block, ONE copy
// into pinned staging, one wait, then the rows into the caller's bitmaps.
int impgpu_album_download_fi(const impgpu_image* album, int bpp, unsigned char* const* bits, const int* pitches) {
    if (!album || !bits || !pitches || (bpp != 24 && bpp != 32) || album->c < 3) return IMP_ERROR_INVALID_ARGS;
    const size_t rowbytes = (size_t)album->w * (bpp / 8);
    for (int i = 0; i < album->frames; i++)
        if (!bits[i] || pitches[i] < 0 || (size_t)pitches[i] < rowbytes) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    const int dpitch = (int)((rowbytes + 3) & ~size_t(3));         // FreeImage's own pitch rule
    const size_t each = ((size_t)dpitch * album->h + 63) & ~size_t(63), total = each * album->frames;
    hipStream_t s = env_stream();
    void* tmp = nullptr;
    if (int rc = dev_alloc(total, &tmp)) return rc;
    int rc = IMP_OK;
    for (int i = 0; i < album->frames && !rc; i++) {
        const View v{album->d + (size_t)i * album->fstride, album->w, album->h, album->c, album->step};
        rc = launch_pack_fi(v, bpp, (uint8_t*)tmp + (size_t)i * each, dpitch, s);
    }
    void *host = nullptr, *token = nullptr;
    if (!rc) rc = stage_begin(total, &host, &token);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(host, tmp, total, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { set_error("hipMemcpyAsync(album_download_fi)", e); rc = IMP_ERROR_DEVICE; }
    }
    dev_free(tmp);
    const int rcw = lane_wait();
    if (rc || rcw) return rc ? rc : rcw;
    for (int i = 0; i < album->frames; i++)
        for (int y = 0; y < album->h; y++)
            std::memcpy(bits[i] + (size_t)y * pitches[i], (const uint8_t*)host + (size_t)i * each + (size_t)y * dpitch, rowbytes);
    return IMP_OK;
}

// Handles [g0, g1) of a call that answers many handles out of one pinned staging buffer: as many as the staging cap takes,
// cut at a handle (a handle past the cap by itself goes alone, as its lone call would) -- impgpu_batch_gif_compose's rule.
// `bytes[k]` is what handle k puts into the buffer (0: refused, it rides along for nothing).
static size_t stage_group_end(const std::vector<size_t>& bytes, size_t g0, size_t cap, size_t* total) {
    size_t g1 = g0, sum = 0;
    while (g1 < bytes.size() && (sum == 0 || !cap || sum + bytes[g1] <= cap)) sum += bytes[g1++];
    *total = sum;
    return g1;
}

// impgpu_album_download_fi for many handles: every accepted frame's flip and repack goes into ONE device block through
// k_pack_fi_mix, one launch per (source channels, bpp) pair present; then one copy into pinned staging, one wait, and the
// rows into the callers' bitmaps.
int impgpu_batch_download_fi(const impgpu_image* const* images, const int* bpps, int count, unsigned char* const* bits,
                             const int* pitches, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 256 || (count > 0 && (!images || !bpps || !bits || !pitches || !codes))) return IMP_ERROR_INVALID_ARGS;
    if (count == 0) return IMP_OK;                                     // nothing asked: answered without a device
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    const unsigned long long launched = t_launches;
    // impgpu_album_download_fi's refusals per handle: nothing of a refused entry is touched
    std::vector<size_t> first((size_t)count), bytes((size_t)count, 0);    // the handle's first frame in bits[]; its bytes in the block
    std::vector<int> dpitch((size_t)count, 0);
    size_t frame0 = 0;
    for (int i = 0; i < count; i++) {
        const impgpu_image* im = images[i];
        first[(size_t)i] = frame0;
        codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!im) continue;
        frame0 += (size_t)im->frames;
        const int bpp = bpps[i];
        if ((bpp != 24 && bpp != 32) || im->c < 3) continue;
        const size_t rowbytes = (size_t)im->w * (bpp / 8);
        bool ok = true;
        for (int f = 0; f < im->frames && ok; f++) {
            const size_t at = first[(size_t)i] + (size_t)f;
            ok = bits[at] && pitches[at] >= 0 && (size_t)pitches[at] >= rowbytes;
        }
        dpitch[(size_t)i] = (int)((rowbytes + 3) & ~size_t(3));    // FreeImage's own pitch rule
        // (what launch_pack_fi refuses of a wrapped BGRA frame: rows off the dword grid)
        if (im->c == 4 && bpp == 32 && (((uintptr_t)im->d | (uintptr_t)im->step | (uintptr_t)im->fstride) & 3)) ok = false;
        if (!ok) continue;
        codes[i] = IMP_OK;
        bytes[(size_t)i] = (((size_t)dpitch[(size_t)i] * im->h + 63) & ~size_t(63)) * (size_t)im->frames;
    }
    const size_t cap = stage_cap();
    hipStream_t s = env_stream();
    for (size_t g0 = 0; g0 < (size_t)count;) {
        size_t total = 0;
        const size_t g1 = stage_group_end(bytes, g0, cap, &total);
        if (total) {
            void *tmp = nullptr, *host = nullptr, *token = nullptr;
            int rc = dev_alloc(total, &tmp);
            if (!rc) {
                Group<PackFiItem> packs[2][2];                              // by source channels (3, 4) and bpp (24, 32)
                size_t at = 0;
                for (size_t i = g0; i < g1; i++) {
                    if (!bytes[i]) continue;
                    const impgpu_image* im = images[i];
                    const size_t each = bytes[i] / (size_t)im->frames;
                    for (int f = 0; f < im->frames; f++, at += each)
                        packs[im->c - 3][bpps[i] == 32].add((int)i, PackFiItem{im->d + (size_t)f * im->fstride, im->w, im->h, im->step,
                                                                              (uint8_t*)tmp + at, dpitch[i]});
                }
                for (int c = 0; c < 2 && !rc; c++)
                    for (int b = 0; b < 2 && !rc; b++)
                        rc = launch_pack_fi_mixed(packs[c][b].items.data(), packs[c][b].size(), c + 3, b ? 32 : 24, s);
                if (!rc) rc = stage_begin(total, &host, &token);
                if (!rc) {
                    const hipError_t e = hipMemcpyAsync(host, tmp, total, hipMemcpyDeviceToHost, s);
                    if (e != hipSuccess) { set_error("hipMemcpyAsync(batch_download_fi)", e); rc = IMP_ERROR_DEVICE; }
                }
                dev_free(tmp);
                const int rcw = lane_wait();
                if (!rc) rc = rcw;
            }
            size_t at = 0;
            for (size_t i = g0; i < g1; i++) {                            // this group's handles fail together; the others stand
                if (!bytes[i]) continue;
                const impgpu_image* im = images[i];
                const size_t each = bytes[i] / (size_t)im->frames, rowbytes = (size_t)im->w * (bpps[i] / 8);
                if (rc) { codes[i] = rc; continue; }
                for (int f = 0; f < im->frames; f++, at += each) {
                    unsigned char* to = bits[first[i] + (size_t)f];
                    const size_t pitch = (size_t)pitches[first[i] + (size_t)f];
                    for (int y = 0; y < im->h; y++) std::memcpy(to + (size_t)y * pitch, (const uint8_t*)host + at + (size_t)y * dpitch[i], rowbytes);
                }
            }
        }
        g0 = g1;
    }
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

// impgpu_album_download for many handles: each handle's block is one copy into its part of ONE pinned staging buffer, all
// of them enqueued before ONE wait; then the rows into the callers' frames.  The fault point impgpu_album_download enters
// is entered per handle that call would take, in handle order, before anything is enqueued.
int impgpu_batch_album_download(const impgpu_image* const* images, int count, unsigned char* const* datas, const int* steps, int* codes) {
    if (count < 0 || count > 256 || (count > 0 && (!images || !datas || !steps || !codes))) return IMP_ERROR_INVALID_ARGS;
    if (count == 0) return IMP_OK;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    TraceRange tr("IMP_STEP_ENCODE");
    std::vector<size_t> first((size_t)count), bytes((size_t)count, 0);
    size_t frame0 = 0;
    for (int i = 0; i < count; i++) {
        const impgpu_image* im = images[i];
        first[(size_t)i] = frame0;
        codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!im) continue;
        frame0 += (size_t)im->frames;
        const size_t rowbytes = (size_t)im->w * im->c;
        bool ok = true;
        for (int f = 0; f < im->frames && ok; f++) {
            const size_t at = first[(size_t)i] + (size_t)f;
            ok = datas[at] && steps[at] >= 0 && (size_t)steps[at] >= rowbytes;
        }
        if (!ok) continue;
        if (fault_hit(IMP_STEP_ENCODE)) { codes[i] = IMP_ERROR_DEVICE; continue; }
        codes[i] = IMP_OK;
        const size_t frame = (size_t)im->step * im->h;
        bytes[(size_t)i] = (((im->frames > 1 ? im->fstride * (size_t)(im->frames - 1) : 0) + frame) + 63) & ~size_t(63);
    }
    const size_t cap = stage_cap();
    hipStream_t s = env_stream();
    for (size_t g0 = 0; g0 < (size_t)count;) {
        size_t total = 0;
        const size_t g1 = stage_group_end(bytes, g0, cap, &total);
        if (total) {
            void *host = nullptr, *token = nullptr;
            int rc = stage_begin(total, &host, &token);
            size_t at = 0;
            for (size_t i = g0; i < g1 && !rc; i++) {
                if (!bytes[i]) continue;
                const impgpu_image* im = images[i];
                const size_t block = (im->frames > 1 ? im->fstride * (size_t)(im->frames - 1) : 0) + (size_t)im->step * im->h;
                const hipError_t e = hipMemcpyAsync((uint8_t*)host + at, im->d, block, hipMemcpyDeviceToHost, s);
                if (e != hipSuccess) { set_error("hipMemcpyAsync(batch_album_download)", e); rc = IMP_ERROR_DEVICE; }
                at += bytes[i];
            }
            const int rcw = lane_wait();
            if (!rc) rc = rcw;
            at = 0;
            for (size_t i = g0; i < g1; i++) {
                if (!bytes[i]) continue;
                const impgpu_image* im = images[i];
                if (rc) { codes[i] = rc; continue; }
                const size_t rowbytes = (size_t)im->w * im->c;
                for (int f = 0; f < im->frames; f++) {
                    unsigned char* to = datas[first[i] + (size_t)f];
                    const size_t dstep = (size_t)steps[first[i] + (size_t)f];
                    const uint8_t* from = (const uint8_t*)host + at + (size_t)f * im->fstride;
                    for (int y = 0; y < im->h; y++) std::memcpy(to + (size_t)y * dstep, from + (size_t)y * im->step, rowbytes);
                }
                at += bytes[i];
            }
        }
        g0 = g1;
    }
    return IMP_OK;
}

int impgpu_calc_perceived_brightness(const impgpu_image* image, float* brightness) {
    if (!image || !brightness) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    TraceRange tr("IMP_STEP_INFO");                                    // bridge.c:659-666
    IMP_FAULT_POINT(IMP_STEP_INFO);
    return launch_brightness(view_of(image), brightness, env_stream());
}

int impgpu_ascii(impgpu_image* image, const char* args, unsigned char* out, long capacity, long* length) {
    static const unsigned char wide[] = "$@B%8&WM#*oahkbdpqwmZO0QLCJUYXzcvunxrjft/\\|()1{}[]?-_+~<>i!lI;:,\"^`'. ";
    static const unsigned char narrow[] = "@%8#*+=-:. ";
    if (!image || !out || !length) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    if (image->c < 3) return IMP_ERROR_INVALID_ARGS;
    const unsigned char* table = (args && !std::strcmp(args, "wide")) ? wide : narrow;
    const int tablelen = (int)std::strlen((const char*)table);
    const float factor = (float)(256.0 / tablelen);
    const long buflen = (long)(image->w + 1) * image->h - 1;
    if (capacity < buflen) return IMP_ERROR_INVALID_ARGS;
    void *dev_table = nullptr, *dev_out = nullptr;
    if (int rc = upload_small(table, (size_t)tablelen + 1, &dev_table, env_stream())) return rc;
    if (int rc = dev_alloc((size_t)buflen + 1, &dev_out)) { dev_free(dev_table); return rc; }
    int rc = launch_ascii(image->d, image->w, image->h, image->c, image->step, (const uint8_t*)dev_table, tablelen, factor,
                          (uint8_t*)dev_out, env_stream());
    if (!rc) {
        hipError_t e = hipMemcpyAsync(out, dev_out, (size_t)buflen, hipMemcpyDeviceToHost, env_stream());
        if (e == hipSuccess) e = hipStreamSynchronize(env_stream());
        if (e != hipSuccess) { set_error("ascii readback", e); rc = IMP_ERROR_DEVICE; }
    }
    dev_free(dev_table);
    dev_free(dev_out);
    if (!rc) *length = buflen;
    return rc;
}

// The json exit of many requests at once: impgpu_calc_perceived_brightness per entry, at most two launches per channel count
// and ONE wait for the call.
int impgpu_batch_calc_perceived_brightness(const impgpu_image* const* images, int count, float* brightness, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 256 || (count > 0 && (!images || !brightness || !codes))) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    TraceRange tr("IMP_STEP_INFO");
    const unsigned long long launched = t_launches;
    // the fault point impgpu_calc_perceived_brightness enters, per entry that call would take, in entry order, before anything
    // is launched (the rule of impgpu_batch_run_ops); an entry whose point fires is left out of the launch
    std::vector<View> views;
    std::vector<int> who;
    views.reserve((size_t)count);
    who.reserve((size_t)count);
    for (int i = 0; i < count; i++) {
        if (!images[i]) { codes[i] = IMP_ERROR_INVALID_ARGS; continue; }
        if (fault_hit(IMP_STEP_INFO)) { codes[i] = IMP_ERROR_DEVICE; continue; }
        views.push_back(view_of(images[i]));
        who.push_back(i);
    }
    const int m = (int)who.size();
    std::vector<float> vals((size_t)m, 0.f);
    std::vector<int> cs((size_t)m, IMP_OK);
    const int rc = launch_brightness_mixed(views.data(), m, vals.data(), cs.data(), env_stream());
    for (int j = 0; j < m; j++) {
        codes[who[(size_t)j]] = rc ? rc : cs[(size_t)j];
        if (!rc && cs[(size_t)j] == IMP_OK) brightness[who[(size_t)j]] = vals[(size_t)j];
    }
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

// The text exit of many requests at once: impgpu_ascii per entry, one launch per channel count, one copy of all texts and ONE wait.
int impgpu_batch_ascii(impgpu_image* const* images, const char* const* args, int count, unsigned char* const* outs,
                       const long* capacities, long* lengths, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 256 || (count > 0 && (!images || !outs || !capacities || !lengths || !codes))) return IMP_ERROR_INVALID_ARGS;
    {
        std::vector<const impgpu_image*> seen;                          // the same handle twice: its frame would be converted twice
        seen.reserve((size_t)count);
        for (int i = 0; i < count; i++) if (images[i]) seen.push_back(images[i]);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return IMP_ERROR_INVALID_ARGS;
    }
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    const unsigned long long launched = t_launches;
    std::vector<AsciiItem> items;
    std::vector<int> who;
    items.reserve((size_t)count);
    who.reserve((size_t)count);
    for (int i = 0; i < count; i++) {
        const impgpu_image* im = images[i];
        // impgpu_ascii's refusals, in its order: nothing of a refused entry is touched
        if (!im || !outs[i] || im->c < 3 || capacities[i] < (long)(im->w + 1) * im->h - 1) { codes[i] = IMP_ERROR_INVALID_ARGS; continue; }
        const char* a = args ? args[i] : nullptr;
        items.push_back(AsciiItem{im->d, im->w, im->h, im->c, im->step, a && !std::strcmp(a, "wide"), outs[i]});
        who.push_back(i);
    }
    const int m = (int)who.size();
    std::vector<int> cs((size_t)m, IMP_OK);
    const int rc = launch_ascii_mixed(items.data(), m, cs.data(), env_stream());
    for (int j = 0; j < m; j++) {
        const int i = who[(size_t)j];
        codes[i] = rc ? rc : cs[(size_t)j];
        if (codes[i] == IMP_OK) lengths[i] = (long)(images[i]->w + 1) * images[i]->h - 1;
    }
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

int impgpu_gray2bgr(impgpu_image** pointer) {
    if (!pointer || !*pointer) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    if ((*pointer)->c != 1) return IMP_OK;
    impgpu_image* out = nullptr;
    Work wk{*pointer, view_of(*pointer)};
    if (int rc = wk.fresh(wk.v.w, wk.v.h, 3, &out)) return rc;
    if (int rc = launch_gray2bgr(wk.to(out), env_stream())) { image_delete(out); return rc; }
    wk.adopt(out);
    *pointer = wk.owner;
    return IMP_OK;
}

static int single_stage(impgpu_image* image, int kind) {
    if (!image) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    if (image->c < 3) return IMP_ERROR_INVALID_ARGS;
    PixelProgram prog;
    Stage s{};
    s.kind = kind;
    prog.stages.push_back(s);
    return launch_pixel_program(image->d, (long long)image->fstride, image->w, image->h, image->c, image->step, image->frames, prog, env_stream());
}
int impgpu_rgb2hsv(impgpu_image* image) { return single_stage(image, ST_RGB2HSV); }
int impgpu_hsv2rgb(impgpu_image* image) { return single_stage(image, ST_HSV2RGB); }

int impgpu_run_ops(impgpu_image** pointer, const impgpu_job* job, const impgpu_config* config, int* step) {
    int dummy;
    if (!step) step = &dummy;
    *step = IMP_STEP_START;
    if (!pointer || !*pointer || !job || !config) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    // bridge.c:361-363 rejects the request while parsing; same limit here
    if (config->max_filters_count > 0 && job->filter_count > config->max_filters_count) return IMP_ERROR_TOO_MUCH_FILTERS;
    Work wk{*pointer, view_of(*pointer)};
    int rc = IMP_OK;
    PixelProgram prog;
    int fused_filters = 0;                                             // leading filters the Resize launch already applied
    bool watermark_done = false;

    *step = IMP_STEP_CROP;                                             // bridge.c:575-586
    if (job->crop) {
        TraceRange tr("IMP_STEP_CROP");
        if (fault_hit(IMP_STEP_CROP)) { rc = IMP_ERROR_DEVICE; goto done; }
        int x, y, w, h;
        rc = crop_geometry(wk.v.w, wk.v.h, job->crop, job->gravity, &x, &y, &w, &h);
        if (rc) goto done;
        wk.v = view_sub(wk.v, x, y, w, h);                             // no copy: the next operator reads the window
    }
    *step = IMP_STEP_RESIZE;                                           // bridge.c:588-604
    if (job->resize) {
        TraceRange tr("IMP_STEP_RESIZE");
        if (fault_hit(IMP_STEP_RESIZE)) { rc = IMP_ERROR_DEVICE; goto done; }
        int w, h, interp;
        rc = resize_geometry(wk.v.w, wk.v.h, job->resize, config->max_target_w, config->max_target_h, job->simple, &w, &h, &interp);
        if (rc) goto done;
        // A thumbnail request whose first filter is a rotation -- and, when that is its only filter, its watermark -- in
        // ONE launch: both ride on the stores of the row-streaming AREA kernel (a lone request is launch-bound: this is a
        // third of its launches and two intermediate frames).  Anything the fused kernel does not take goes step by step.
        rc = IMP_ERROR_UNSUPPORTED;
        bool with_wm = false;
        if (const int rot = fused_turn(wk.v, wk.count(), w, h, interp, job, config, &with_wm)) {
            const bool swap = rot != 180;
            const int fw = swap ? h : w, fh = swap ? w : h;
            OverlayArgs wm{};
            if (with_wm && overlay_args(config, fw, fh, &wm) != IMP_OK) with_wm = false;   // (it fails at the watermark step)
            impgpu_image* out = nullptr;
            rc = wk.fresh(fw, fh, wk.v.c, &out);
            if (rc) goto done;
            Frames f = wk.to(out);
            f.dw = w; f.dh = h;                                        // the resized geometry; `out` is the turned frame
            rc = launch_area_rotate(f, rot, with_wm ? &wm : nullptr, env_stream());
            if (rc == IMP_OK) { wk.adopt(out); fused_filters = 1; watermark_done = with_wm; }
            else image_delete(out);
        }
        if (rc == IMP_ERROR_UNSUPPORTED) rc = do_resize(wk, w, h, interp);
        if (rc) goto done;
    }
    *step = IMP_STEP_FILTERING;                                        // bridge.c:606-627
    trace_push("IMP_STEP_FILTERING");
    if ((wk.v.c == 1 || job->filter_count > 0) && fault_hit(IMP_STEP_FILTERING)) { rc = IMP_ERROR_DEVICE; trace_pop(); goto done; }
    if (wk.v.c == 1) {
        impgpu_image* out = nullptr;
        rc = wk.fresh(wk.v.w, wk.v.h, 3, &out);
        if (rc) { trace_pop(); goto done; }
        rc = launch_gray2bgr(wk.to(out), env_stream());
        if (rc) { image_delete(out); trace_pop(); goto done; }
        wk.adopt(out);
    }
    for (int i = fused_filters; i < job->filter_count && !rc; i++) rc = do_filter(wk, job->filters[i], config->allow_experiments, prog);
    if (!rc) rc = flush_program(wk, prog);
    trace_pop();
    if (rc) goto done;
    *step = IMP_STEP_WATERMARK;                                        // bridge.c:629-640
    if (config->watermark) {
        TraceRange tr("IMP_STEP_WATERMARK");
        if (fault_hit(IMP_STEP_WATERMARK)) { rc = IMP_ERROR_DEVICE; goto done; }
        if (!watermark_done) rc = do_watermark(wk, config);
        if (rc) goto done;
    }
    if (job->need_flatten && wk.v.c == 4) {                            // bridge.c:642-656
        rc = launch_blend_paper(wk.px(), wk.stride(), wk.v.w, wk.v.h, wk.v.step, wk.count(), env_stream());
        if (rc) goto done;
    }
    rc = materialize(wk);
    if (!rc) *step = IMP_STEP_INFO;
done:
    *pointer = wk.owner;
    return rc;
}

int impgpu_batch_run_ops(impgpu_image** images, const impgpu_job* jobs, const impgpu_config* const* configs, int count,
                         int* codes, int* steps, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 4096 || (count > 0 && (!images || !jobs || !configs || !codes || !steps))) return IMP_ERROR_INVALID_ARGS;
    {
        std::vector<const impgpu_image*> seen;                          // the same handle twice: one request would free the other's frame
        seen.reserve((size_t)count);
        for (int i = 0; i < count; i++) if (images[i]) seen.push_back(images[i]);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return IMP_ERROR_INVALID_ARGS;
    }
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) { codes[i] = rc; steps[i] = IMP_STEP_START; }
        return rc;
    }
    const unsigned long long launched = t_launches;
    Batch b{images, jobs, configs, count, codes, steps, env_stream()};
    b.runs.resize((size_t)count);
    int albums = 0;
    for (int i = 0; i < count; i++) albums += images[i] && images[i]->frames > 1 && images[i]->c >= 3;
    b.share_albums = albums >= 2;
    for (int i = 0; i < count; i++) b.admit(i);
    b.resize_round();
    b.promote_gray();
    // one round more than the longest chain: the windows left behind it; it launches nothing unless such a request exists
    for (size_t r = 0; r <= b.rounds; r++) b.segment_round(r);
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

// ------------------------------------------------------------------ batch entry points
int impgpu_batch_cv_resize(const void* src, long long src_frame_stride, int src_width, int src_height, int src_step,
                           void* dst, long long dst_frame_stride, int dst_width, int dst_height, int dst_step,
                           int channels, int count, int interpolation, void* stream) {
    if (!src || !dst || (channels != 1 && channels != 3 && channels != 4)) return IMP_ERROR_INVALID_ARGS;
    if (!view_fits(src_width, src_height, channels, src_step) || !view_fits(dst_width, dst_height, channels, dst_step)) return IMP_ERROR_INVALID_ARGS;
    if (count < 0 || count > 65535 || (count > 1 && (src_frame_stride < 0 || dst_frame_stride < 0))) return IMP_ERROR_INVALID_ARGS;
    if (interpolation < IMP_INTER_NN || interpolation > IMP_INTER_LANCZOS4) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    Frames f{};
    f.src = (const uint8_t*)src; f.src_stride = src_frame_stride;
    f.v = View{(const uint8_t*)src, src_width, src_height, channels, src_step};
    f.dst = (uint8_t*)dst; f.dst_stride = dst_frame_stride; f.dw = dst_width; f.dh = dst_height; f.dstep = dst_step;
    f.count = count;
    return launch_cv_resize(f, interpolation, stream ? (hipStream_t)stream : env_stream());
}

int impgpu_batch_resize_mixed(const impgpu_resize_item* items, int count, int channels, int simple, void* stream) {
    return impgpu_batch_resize_mixed_ex(items, count, channels, simple, stream, nullptr);
}

int impgpu_batch_resize_mixed_ex(const impgpu_resize_item* items, int count, int channels, int simple, void* stream, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || (count > 0 && !items) || (channels != 1 && channels != 3 && channels != 4)) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++)                                     // (again in the launcher; here so that it answers without a device)
        if (!items[i].src || !items[i].dst || !view_fits(items[i].src_width, items[i].src_height, channels, items[i].src_step) ||
            !view_fits(items[i].dst_width, items[i].dst_height, channels, items[i].dst_step))
            return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    static_assert(sizeof(MixFrame) == sizeof(impgpu_resize_item) && offsetof(MixFrame, dst) == offsetof(impgpu_resize_item, dst),
                  "MixFrame mirrors impgpu_resize_item");
    const unsigned long long launched = t_launches;
    const int rc = launch_resize_mixed(reinterpret_cast<const MixFrame*>(items), count, channels, simple,
                                       stream ? (hipStream_t)stream : env_stream());
    if (launches) *launches = (int)(t_launches - launched);
    return rc;
}

int impgpu_batch_resize_rotate_watermark(const void* src, long long src_frame_stride, int src_width, int src_height, int src_step,
                                         void* dst, long long dst_frame_stride, int dst_step,
                                         int resize_width, int resize_height, int rotate,
                                         const impgpu_config* config, int channels, int count, void* stream) {
    if (!src || !dst || !config || (channels != 3 && channels != 4)) return IMP_ERROR_INVALID_ARGS;
    if (rotate != 0 && rotate != 90 && rotate != 180 && rotate != 270) return IMP_ERROR_INVALID_ARGS;
    if (!view_fits(src_width, src_height, channels, src_step) || resize_width <= 0 || resize_height <= 0 ||
        !view_fits(rotate == 90 || rotate == 270 ? resize_height : resize_width, rotate == 90 || rotate == 270 ? resize_width : resize_height, channels, dst_step))
        return IMP_ERROR_INVALID_ARGS;
    if (count < 0 || count > 65535 || (count > 1 && (src_frame_stride < 0 || dst_frame_stride < 0))) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : env_stream();
    const int interp = (resize_width > src_width || resize_height > src_height) ? IMP_INTER_CUBIC : IMP_INTER_AREA;  // bridge.c:190
    const bool swap = rotate == 90 || rotate == 270;
    const int fw = swap ? resize_height : resize_width, fh = swap ? resize_width : resize_height;
    if (dst_step < fw * channels) return IMP_ERROR_INVALID_ARGS;

    Frames rs{};
    rs.src = (const uint8_t*)src; rs.src_stride = src_frame_stride;
    rs.v = View{(const uint8_t*)src, src_width, src_height, channels, src_step};
    rs.count = count;
    rs.dw = resize_width; rs.dh = resize_height;
    void* mid = nullptr;
    int rc;
    rc = IMP_ERROR_UNSUPPORTED;
    bool watermark_done = false;
    if (interp == IMP_INTER_AREA && swap && resize_width * 2 == src_width && resize_height * 2 == src_height) {
        // exact 2x2 box + quarter turn: one pass, the half-size intermediate never reaches HBM -- and with a BGRA overlay
        // (4-byte aligned rows) the Watermark step rides on the same kernel's stores
        Frames fz = rs;
        fz.dst = (uint8_t*)dst; fz.dst_stride = dst_frame_stride; fz.dstep = dst_step; fz.dw = fw; fz.dh = fh;
        OverlayArgs wm{};
        const bool fuse = channels == 4 && bgra_overlay(config->watermark);
        if (fuse && (rc = overlay_args(config, fw, fh, &wm)) != IMP_OK) return rc;
        rc = launch_area2x2_rotate(fz, rotate, fuse ? &wm : nullptr, s);
        watermark_done = fuse && rc == IMP_OK;
    }
    if (rc == IMP_ERROR_UNSUPPORTED && interp == IMP_INTER_AREA) {
        // any other shrink, BGRA or BGR: the rotate and the watermark ride on the store phase of the row-streaming AREA kernel
        Frames fz = rs;
        fz.dst = (uint8_t*)dst; fz.dst_stride = dst_frame_stride; fz.dstep = dst_step;
        OverlayArgs wm{};
        const bool fuse = bgra_overlay(config->watermark);
        if (fuse && (rc = overlay_args(config, fw, fh, &wm)) != IMP_OK) return rc;
        rc = launch_area_rotate(fz, rotate, fuse ? &wm : nullptr, s);
        watermark_done = fuse && rc == IMP_OK;
    }
    if (rc != IMP_ERROR_UNSUPPORTED) {
        // fused path taken (or failed with a device error)
    } else if (rotate == 0) {
        rs.dst = (uint8_t*)dst; rs.dst_stride = dst_frame_stride; rs.dstep = dst_step;
        rc = launch_cv_resize(rs, interp, s);
    } else {
        const int mstep = aligned_step(resize_width, channels);
        const long long mstride = ((long long)mstep * resize_height + 15) & ~15LL;
        rc = dev_alloc_on((size_t)mstride * count + 16, &mid, s);
        if (rc) return rc;
        rs.dst = (uint8_t*)mid; rs.dst_stride = mstride; rs.dstep = mstep;
        rc = launch_cv_resize(rs, interp, s);
        if (!rc) {
            Frames rt{};
            rt.src = (const uint8_t*)mid; rt.src_stride = mstride;
            rt.v = View{(const uint8_t*)mid, resize_width, resize_height, channels, mstep};
            rt.dst = (uint8_t*)dst; rt.dst_stride = dst_frame_stride; rt.dw = fw; rt.dh = fh; rt.dstep = dst_step;
            rt.count = count;
            rc = launch_rotate(rt, rotate, s);
        }
    }
    if (!rc && config->watermark && !watermark_done) {
        OverlayArgs wm{};
        rc = overlay_args(config, fw, fh, &wm);
        if (!rc) rc = launch_blend_over((uint8_t*)dst, dst_frame_stride, fw, fh, channels, dst_step, count, config->watermark,
                                        wm.rx, wm.ry, wm.maxcol, wm.maxrow, wm.alpha, s);
    }
    if (mid) dev_free_on(mid, s);       // no host wait: parked behind an event when `s` is the caller's stream
    return rc;
}

int impgpu_batch_filters(void* frames, long long frame_stride, int width, int height, int channels, int step, int count,
                         const char* const* filters, int filter_count, int allow_experiments, void* stream) {
    if (!frames || !filters || filter_count < 0 || (channels != 3 && channels != 4) || !view_fits(width, height, channels, step)) return IMP_ERROR_INVALID_ARGS;
    if (count < 0 || count > 65535 || (count > 1 && frame_stride < 0)) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    PixelProgram prog;
    for (int i = 0; i < filter_count; i++) {
        FilterPlan plan;
        if (int rc = filter_plan(filters[i], allow_experiments, channels, width, height, &plan, &prog)) return rc;
        if (plan.cls != FC_POINTWISE && plan.cls != FC_NOOP) return IMP_ERROR_UNSUPPORTED;
    }
    return launch_pixel_program((uint8_t*)frames, frame_stride, width, height, channels, step, count, prog,
                                stream ? (hipStream_t)stream : env_stream());
}

}  // extern "C"
