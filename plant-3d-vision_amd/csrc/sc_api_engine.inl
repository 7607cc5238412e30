// Part of spacecarve.hip (included there): the C ABI, first half -- engines (sc_create* .. sc_set_option, streams) and views
// (sc_process_view*, sc_process_png_views, sc_process_views_device, sc_average_labels).  Each entry cites the cl.py line
// it replaces in include/spacecarve.h.

extern "C" {

int sc_abi_version(void) { return SC_ABI_VERSION; }

const char *sc_last_error(void) { return g_err.c_str(); }

int sc_device_count(int *count) {
    if (!count) return fail(SC_ERR_INVALID, "null count");
    *count = 0;
    int n = 0;
    hipError_t he = hipGetDeviceCount(&n);
    if (he != hipSuccess) return fail(SC_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(he));
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) continue;
        if (strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;  // other devices are simply not ours
    }
    *count = ok;
    return SC_OK;
}

int sc_create(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, const float origin[3],
              float voxel_size, int mode, float default_value, int device) {
    return create(out, nx, ny, nz, 0, 1, nx, origin, voxel_size, mode, default_value, device);
}

int sc_create_slab(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t i0, int64_t i1,
                   const float origin[3], float voxel_size, int mode, float default_value,
                   int device) {
    if (i0 < 0 || i1 > nx || i0 >= i1) return fail(SC_ERR_INVALID, "bad slab [%lld, %lld)", (long long)i0, (long long)i1);
    return create(out, nx, ny, nz, i0, 1, i1 - i0, origin, voxel_size, mode, default_value, device);
}

int sc_create_cyclic(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t first, int64_t stride,
                     const float origin[3], float voxel_size, int mode, float default_value,
                     int device) {
    if (stride < 1 || first < 0 || first >= stride || first >= nx)
        return fail(SC_ERR_INVALID, "bad plane set (first %lld, stride %lld)", (long long)first, (long long)stride);
    int64_t planes = (nx - first + stride - 1) / stride;
    return create(out, nx, ny, nz, first, stride, planes, origin, voxel_size, mode, default_value, device);
}

// What cl.py:29-30 does at import -- the context and the queue -- without blocking the importer: a thread of the library's
// initialises the runtime on `device` and creates the device's first non-blocking stream (84-147 ms in a fresh process),
// which the first engine on that device then takes from the idle-stream list.  Returns at once; errors are the first
// engine's to report (it runs the same calls).
int sc_prewarm(int device) {
    if (device < 0 || device >= 64) return fail(SC_ERR_INVALID, "device %d", device);
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        if (g_prewarm_running[device]) return SC_OK;
        for (auto &p : g_stream_pool)
            if (p.first == device) return SC_OK;  // a stream is waiting already
        g_prewarm_running[device] = 1;
    }
    try {
        std::thread([device]() {
            hipStream_t s = nullptr;
            int n = 0;
            bool ok = hipGetDeviceCount(&n) == hipSuccess && device < n && hipSetDevice(device) == hipSuccess &&
                      hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
            std::lock_guard<std::mutex> lk(g_stream_mu);
            if (ok) g_stream_pool.emplace_back(device, s);
            g_prewarm_running[device] = 0;
            g_prewarm_cv.notify_all();
        }).detach();
    } catch (...) {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        g_prewarm_running[device] = 0;
        g_prewarm_cv.notify_all();
    }
    return SC_OK;
}

// A process must not run its exit handlers -- the runtime's among them -- while a prewarm thread is still inside hipInit:
// whoever started one waits for it here before the interpreter goes down (plant-3d-vision_amd/_native.py registers this
// with atexit); returns at once when none is running.
void sc_prewarm_wait(void) {
    std::unique_lock<std::mutex> lk(g_stream_mu);
    g_prewarm_cv.wait(lk, [] {
        for (int d = 0; d < 64; ++d)
            if (g_prewarm_running[d]) return false;
        return true;
    });
}

int sc_create_ex(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t first, int64_t stride, int64_t planes,
                 const float origin[3], float voxel_size, int mode, float default_value, int device, int flags) {
    if (flags & ~SC_CREATE_DEFERRED) return fail(SC_ERR_INVALID, "unknown creation flags %d", flags);
    return create(out, nx, ny, nz, first, stride, planes, origin, voxel_size, mode, default_value, device,
                  (flags & SC_CREATE_DEFERRED) != 0);
}

// Diagnostic: out[0] = milliseconds the device half of the engine's set-up took (on its own thread when the engine was
// created deferred), out[1] = milliseconds the first call that needed the device waited for that thread (0: it had
// finished, or the engine was not deferred).  Waits for the set-up.
int sc_setup_times(sc_engine *e, double out[2]) {
    if (!e || !out) return fail(SC_ERR_INVALID, "null argument");
    int rc = wait_setup(e);
    if (rc) return rc;
    out[0] = e->setup_ms;
    out[1] = e->setup_waited_ms;
    return SC_OK;
}

void sc_destroy(sc_engine *e) {
    if (!e) return;
    if (e->setup_pending && e->setup_thread.joinable()) e->setup_thread.join();
    e->setup_pending = false;
    if (e->setup_rc != SC_OK) {  // the device half never came up: nothing but host memory to give back
        if (e->own_stream) give_stream_back(e->device, e->own_stream);
        delete e;
        return;
    }
    (void)hipSetDevice(e->device);
    if (e->stream) (void)schost::wait_stream(e->stream);  // (before anything is freed)
    const int device = e->device;
    const hipStream_t own = e->own_stream;
    delete e;  // every buffer and event goes with its owner
    if (own) {
        (void)schost::wait_stream(own);  // (the engine may have worked on a caller's stream: its own is idle now)
        give_stream_back(device, own);
    }
}

int sc_clear(sc_engine *e) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    int rc = use_device(e);
    if (rc) return rc;
    e->pending.clear();
    e->hp_pending.clear();
    e->hb[e->hb_cur].used = 0;  // (nothing of it was uploaded)
    e->deferred.on = false;
    e->dead_clean = false;  // the labels go back to default_value: no brick is known to be all -1
    e->sparse_exact = false;
    arena_reset(e);
    // the views of an open SC_KERNEL_STEP window are gone: no sample for them
    if (e->step_start) e->event_pool.push_back(std::move(e->step_start));
    e->fresh = true;  // materialised lazily: a fused launch never needs to read it
    return SC_OK;
}

int sc_set_option(sc_engine *e, int key, int64_t value) {
    if (e) {
        int rcw = wait_setup(e);  // (some keys create events or move buffers)
        if (rcw) return rcw;
    }
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    switch (key) {
        case SC_OPT_VIEWS_PER_LAUNCH:
            if (value < 0) return fail(SC_ERR_INVALID, "views_per_launch must be >= 0");
            e->views_per_launch = value;
            return SC_OK;
        case SC_OPT_VIEW_ORDER:
            if (value != 0 && value != 1) return fail(SC_ERR_INVALID, "view_order must be 0 or 1");
            e->view_order = value;
            return SC_OK;
        case SC_OPT_TIME_KERNELS:
            e->time_kernels = value == 2 ? 2 : (value ? 1 : 0);
            return SC_OK;
        case SC_OPT_COMPACT:
            e->compact = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_DENSE_VIEWS:
            if (value < 1 || value > 64) return fail(SC_ERR_INVALID, "dense_views must be in [1, 64]");
            e->dense_views = value;
            return SC_OK;
        case SC_OPT_STAGE1_VIEWS:
            if (value < 1 || value > 4096) return fail(SC_ERR_INVALID, "stage1_views must be in [1, 4096]");
            e->stage1_views = value;
            return SC_OK;
        case SC_OPT_BRICK:
            e->brick = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_FULL_BRICKS:
            e->full_bricks = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_AVG_TILE_F32:
            e->avg_tile_f32 = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_AVG_BRICK:
            e->avg_brick = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_PACK_ROWS:
            if (value != 0 && value != 1 && value != 2 && value != 3 && value != 4 && value != 8)
                return fail(SC_ERR_INVALID, "pack_rows must be 0, 1, 2, 3, 4 or 8");
            e->pack_rows = value;
            return SC_OK;
        case SC_OPT_VIEW_BRICK:
            e->view_brick = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_RESERVE_EVENTS: {
            if (value < 0 || value > 65536) return fail(SC_ERR_INVALID, "reserve_events must be in [0, 65536]");
            int rc = use_device(e);
            if (rc) return rc;
            while ((int64_t)e->event_pool.size() < value) {
                Event ev;
                HIP_TRY(hipEventCreate(ev.out()));
                e->event_pool.push_back(std::move(ev));
            }
            return SC_OK;
        }
        case SC_OPT_PACK_RIDE:
            e->pack_ride = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_PACK_REACH:
            e->pack_reach = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_FLAG_VIEWS:
            if (value < 0) return fail(SC_ERR_INVALID, "flag_views must be >= 0");
            e->flag_views = value;
            return SC_OK;
        case SC_OPT_BULK_MIN:
            if (value < 0 || value > 256) return fail(SC_ERR_INVALID, "bulk_min must be in [0, 256]");
            e->bulk_min = value;
            return SC_OK;
        case SC_OPT_UNIT_CULL:
            if (value < 0 || value > 2) return fail(SC_ERR_INVALID, "unit_cull must be 0, 1 or 2");
            e->unit_cull = value;
            return SC_OK;
        case SC_OPT_BULK_LIVE:
            if (value < 0 || value > 16) return fail(SC_ERR_INVALID, "bulk_live must be in [0, 16]");
            e->bulk_live = value;
            return SC_OK;
        case SC_OPT_BULK_FLOOR:
            if (value < 0 || value > 0x7fffffffLL) return fail(SC_ERR_INVALID, "bulk_floor must be in [0, 2^31)");
            e->bulk_floor = value;
            return SC_OK;
        case SC_OPT_LATE_ROAD:
            e->late_road = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_SAFE_KERNELS:
            e->safe_kernels = value ? 1 : 0;
            return SC_OK;
        // Retired in round 6: knobs whose sweeps are settled (profiles/r05_sweep_defaults.json moved no
        // scene by 1 % on them) are fixed at their defaults; the keys stay valid -- accepted, no effect -- because the
        // numbers are part of the ABI (spacecarve_tuning.h)
        case SC_OPT_LIST_BLOCKS:  // fixed at 2048
        case SC_OPT_STAGE2_VIEWS:  // fixed at 0 (no such stage)
        case SC_OPT_STAGE1_STORE_SHARE:  // fixed at 5
        case SC_OPT_STAGE1_LIST_BLOCKS:  // fixed at 1280
        case SC_OPT_DEFER_SHARE:  // fixed at 16
        case SC_OPT_DEFER_STORES:  // fixed at 1536
        case SC_OPT_STAGE1_VOXELS:  // fixed at 2
        case SC_OPT_FINAL_VOXELS:  // fixed at 2
        case SC_OPT_FILL_BLOCKS:  // fixed at 256
        case SC_OPT_BRICK_WALKERS:  // fixed at 1280
        case SC_OPT_VIEW_GROUP:  // fixed at 2
        case SC_OPT_ITEM_BIAS:  // fixed at 12
        case SC_OPT_SPEC_SHARE:  // fixed at 3
        case SC_OPT_SPEC_BLOCKS:  // fixed at 64
        case SC_OPT_UNIT_BLOCKS:  // fixed at 512
        case SC_OPT_DENSE_EXTRA:  // fixed at 1
            return SC_OK;
        case SC_OPT_LDS_TILES:  // the experiment was measured and removed (DESIGN_APPENDIX.md 12): accepted, no effect
            return SC_OK;
        case SC_OPT_HOST_PACK:
            if (!e->hp_pending.empty()) return fail(SC_ERR_STATE, "host-packed views are pending: flush first");
            e->host_pack = value ? 1 : 0;
            return SC_OK;
        case SC_OPT_HOST_THREADS:
            if (value < 0 || value > 256) return fail(SC_ERR_INVALID, "host_threads must be in [0, 256]");
            schost::pool_set_threads((int)value);  // process-wide; takes effect before the pool's first use
            return SC_OK;
        case SC_OPT_LIST_CAP:
            if (value < 0 || value > 0x7fffffffLL) return fail(SC_ERR_INVALID, "list_cap must be in [0, 2^31)");
            e->list_cap = value;
            return SC_OK;
        case SC_OPT_MAX_PENDING:
            if (value < 1) return fail(SC_ERR_INVALID, "max_pending must be >= 1");
            e->max_pending = value;
            return SC_OK;
        default:
            return fail(SC_ERR_INVALID, "unknown option %d", key);
    }
}

int sc_set_lut(sc_engine *e, const float *lut256) {
    if (!e || !lut256) return fail(SC_ERR_INVALID, "null argument");
    if (e->mode != SC_MODE_AVERAGE) return fail(SC_ERR_STATE, "the table belongs to averaging engines");
    int rc = use_device(e);
    if (rc) return rc;
    rc = flush(e);  // views already enqueued keep the old table
    if (rc) return rc;
    HIP_TRY(schost::wait_stream(e->stream));
    if (!e->lut_dev) HIP_TRY(sc_dev_malloc(e->lut_dev.out(), 256 * sizeof(float)));
    HIP_TRY(hipMemcpy(e->lut_dev, lut256, 256 * sizeof(float), hipMemcpyHostToDevice));
    return SC_OK;
}

int sc_set_stream(sc_engine *e, void *hip_stream) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    int rc = use_device(e);
    if (rc) return rc;
    rc = flush(e);
    if (rc) return rc;
    HIP_TRY(schost::wait_stream(e->stream));
    e->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : e->own_stream;
    return SC_OK;
}

int sc_order_after(sc_engine *e, void *producer_stream) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    int rc = use_device(e);
    if (rc) return rc;
    // NULL is the legacy default stream here (torch's default stream has handle 0); the engine's own
    // stream is non-blocking, so it does NOT synchronise with that stream by itself
    // (the handle 0 itself: hipStreamLegacy is not understood by every runtime this library meets --
    // torch's bundled one crashed on it)
    hipStream_t prod = static_cast<hipStream_t>(producer_stream);
    if (prod != nullptr && prod == e->stream) return SC_OK;  // same stream: already in order
    return order_streams(prod, e->stream, "ordering after the producer stream failed");
}

int sc_order_before(sc_engine *e, void *consumer_stream) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    int rc = use_device(e);
    if (rc) return rc;
    hipStream_t cons = static_cast<hipStream_t>(consumer_stream);
    if (cons != nullptr && cons == e->stream) return SC_OK;  // same stream: already in order
    return order_streams(e->stream, cons, "ordering the consumer stream behind the engine failed");
}

int sc_process_view(sc_engine *e, const float K[4], const float R[9], const float t[3],
                    const void *mask, int H, int W, int mask_dtype, int64_t row_stride_bytes) {
    int rc = check_view_args(e, K, R, t, mask, H, W);
    if (rc) return rc;
    rc = check_dtype(e, mask_dtype);
    if (rc) return rc;
    rc = use_device(e);
    if (rc) return rc;
    rc = materialize_deferred(e);  // a device batch waiting for its flush: packed now, order as given
    if (rc) return rc;
    size_t es = elem_size(mask_dtype);
    size_t row = (size_t)W * es;
    if (row_stride_bytes == 0) row_stride_bytes = (int64_t)row;
    if (row_stride_bytes < (int64_t)row) return fail(SC_ERR_INVALID, "row stride smaller than a row");
    if (e->mode == SC_MODE_CARVE && e->host_pack) {
        // the caller's buffer is consumed here (its bits are in the arena when this returns)
        rc = enqueue_hostbits(e, K, R, t, mask, H, W, mask_dtype, row_stride_bytes);
        if (rc) return rc;
        return after_enqueue(e);
    }
    size_t bytes = row * (size_t)H;
    rc = ensure_slots(e, bytes);
    if (rc) return rc;
    int s = e->next_slot;
    e->next_slot = (s + 1) % kSlots;
    if (e->slot_armed[s]) {
        HIP_TRY(schost::wait_event(e->slot_ev[s]));
        e->slot_armed[s] = false;
    }
    void *pin = e->slot[s].pin, *raw = e->slot[s].raw;
    // consume the caller's buffer now (tight rows in the pinned slot)
    if (row_stride_bytes == (int64_t)row) {
        memcpy(pin, mask, bytes);
    } else {
        for (int r = 0; r < H; ++r)
            memcpy(static_cast<char *>(pin) + (size_t)r * row, static_cast<const char *>(mask) + (size_t)r * row_stride_bytes, row);
    }
    // float32 masks read row-major are not re-laid: the slot's pixels go straight to the arena, where the view reads them
    const bool plain = e->mode != SC_MODE_CARVE && mask_dtype != SC_MASK_U8_LUT && !e->avg_tile_f32;
    if (plain) {
        rc = arena_alloc(e, bytes, &raw);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(raw, pin, bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->slot_ev[s], e->stream));
    e->slot_armed[s] = true;
    if (plain) {
        ViewDesc d;
        fill_desc(e, d, K, R, t, raw, H, W);
        e->pending.push_back(d);
    } else if (e->mode == SC_MODE_CARVE) {
        rc = enqueue_pack(e, 1, K, R, t, raw, H, W, mask_dtype, (int64_t)row, (int64_t)bytes);
    } else if (mask_dtype == SC_MASK_U8_LUT) {
        rc = enqueue_tiles(e, kFormU8Strips, 1, K, R, t, raw, H, W, (int64_t)row, (int64_t)bytes);
    } else {
        rc = enqueue_tiles(e, kFormF32Tiles, 1, K, R, t, raw, H, W, (int64_t)row, (int64_t)bytes);
    }
    return rc ? rc : after_enqueue(e);
}

int sc_process_views(sc_engine *e, int V, const float *K, const float *R, const float *t,
                     const void *const *masks, int H, int W, int mask_dtype,
                     int64_t row_stride_bytes) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    if (V < 0 || (V > 0 && (!K || !R || !t || !masks))) return fail(SC_ERR_INVALID, "bad view batch");
    for (int q = 0; q < V; ++q) {
        int rc = sc_process_view(e, K + 4 * q, R + 9 * q, t + 3 * q, masks[q], H, W, mask_dtype,
                                 row_stride_bytes);
        if (rc) return rc;
    }
    return SC_OK;
}

int sc_process_png_views(sc_engine *e, int V, const float *K, const float *R, const float *t, const void *const *png,
                         const int64_t *sizes, int invert, int threads) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    if (V < 0 || (V > 0 && (!K || !R || !t || !png || !sizes))) return fail(SC_ERR_INVALID, "bad view batch");
    if (V == 0) return SC_OK;
    if (e->mode != SC_MODE_CARVE) return fail(SC_ERR_STATE, "encoded masks are carve masks (the averaging path converts pixels on the host)");
    std::vector<int> Ws((size_t)V), Hs((size_t)V);
    std::vector<size_t> offs((size_t)V);
    size_t total = 0;
    for (int q = 0; q < V; ++q) {
        if (!png[q]) return fail(SC_ERR_INVALID, "null file %d", q);
        if (sc_png_info(png[q], sizes[q], &Ws[(size_t)q], &Hs[(size_t)q]) != SC_OK)
            return fail(SC_ERR_INVALID, "file %d: %s", q, sc_png_last_error());
        // the limits check_view_args puts on a mask, before a pixel buffer of that size is asked for
        if (Ws[(size_t)q] <= 0 || Hs[(size_t)q] <= 0 || Ws[(size_t)q] > (1 << 24) || Hs[(size_t)q] > (1 << 24) ||
            (int64_t)Ws[(size_t)q] * Hs[(size_t)q] > (int64_t)1 << 31)
            return fail(SC_ERR_INVALID, "file %d: a %d x %d mask is beyond the limits of a view", q, Ws[(size_t)q], Hs[(size_t)q]);
        offs[(size_t)q] = total;
        total += ((size_t)Hs[(size_t)q] * (size_t)((Ws[(size_t)q] + kTile - 1) / kTile) * 4 + 255) & ~(size_t)255;
    }
    // An engine whose device half is still coming up (sc_create_ex, SC_CREATE_DEFERRED): the files are decoded into
    // plain host memory beside it and copied to the page-locked arena once the device is there -- 14 MB, 2 ms, against
    // the 15 ms of decoding that would otherwise wait for 130-240 ms of runtime set-up
    const bool beside_setup = e->setup_pending;
    std::vector<char> heap;
    int rc = SC_OK;
    char *base = nullptr;
    if (beside_setup) {
        try {
            heap.resize(total);
        } catch (...) {
            return fail(SC_ERR_NOMEM, "out of host memory while decoding the masks");
        }
        base = heap.data();
    } else {
        rc = use_device(e);
        if (rc) return rc;
        rc = materialize_deferred(e);
        if (rc) return rc;
        rc = hostbits_reserve(e, total, &base);  // one reservation: the arena does not move while the threads write
        if (rc) return rc;
    }
    // decode + pack, a file per thread at a time.  Threads of this call's own (16 by default: inflate is the floor
    // of the files -> volume time, ~1.3 ms per mask and thread, and the pool's 8 are sized for the per-mask hand-overs)
    int nth = threads > 0 ? threads : 16;
    nth = std::min(std::min(nth, V), 64);
    std::atomic<int> next{0}, bad{-1};
    std::atomic<bool> nomem{false};
    const uint8_t flip = invert ? 255 : 0;
    // (nothing may leave a thread function or this C entry point as an exception -- std::terminate: the pixel buffer's
    // allocation and the threads' creation are caught and reported as SC_ERR_NOMEM)
    auto work = [&]() {
        try {
            std::vector<uint8_t> pix;
            for (;;) {
                const int q = next.fetch_add(1, std::memory_order_relaxed);
                if (q >= V || bad.load(std::memory_order_relaxed) >= 0) return;
                const int W = Ws[(size_t)q], H = Hs[(size_t)q];
                pix.resize((size_t)W * H);
                if (sc_png_decode_gray8(png[q], sizes[q], pix.data(), W, H) != SC_OK) {
                    int expect = -1;
                    bad.compare_exchange_strong(expect, q);
                    return;
                }
                schost::pack_rows(pix.data(), W, W, 0, H, reinterpret_cast<uint32_t *>(base + offs[(size_t)q]), (W + kTile - 1) / kTile, 1, flip);
            }
        } catch (...) {
            nomem.store(true);
            int expect = -1;
            bad.compare_exchange_strong(expect, V);  // stops the others
        }
    };
    {
        std::vector<std::thread> pool;
        try {
            pool.reserve((size_t)nth);
            for (int i = 1; i < nth; ++i) pool.emplace_back(work);
        } catch (...) {
            // (fewer threads than asked for: the ones that exist and this one do the work)
        }
        work();
        for (auto &th : pool) th.join();
    }
    if (nomem.load()) {
        if (!beside_setup) e->hb[e->hb_cur].used -= total;
        return fail(SC_ERR_NOMEM, "out of host memory while decoding the masks");
    }
    if (bad.load() >= 0) {
        if (!beside_setup) e->hb[e->hb_cur].used -= total;  // nothing of this call stays
        return fail(SC_ERR_INVALID, "file %d could not be decoded", bad.load());
    }
    if (beside_setup) {
        rc = use_device(e);  // joins the set-up
        if (rc) return rc;
        rc = materialize_deferred(e);
        if (rc) return rc;
        char *pinned = nullptr;
        rc = hostbits_reserve(e, total, &pinned);
        if (rc) return rc;
        memcpy(pinned, heap.data(), total);
        base = pinned;
    }
    const uint64_t base_off = (uint64_t)(base - e->hb[e->hb_cur].pin);
    for (int q = 0; q < V; ++q) {
        rc = hostbits_push_view(e, K + 4 * q, R + 9 * q, t + 3 * q, base_off + offs[(size_t)q], Hs[(size_t)q], Ws[(size_t)q]);
        if (rc) return rc;
    }
    return after_enqueue(e);
}

int sc_process_views_device(sc_engine *e, int V, const float *K, const float *R, const float *t,
                            const void *masks_dev, int H, int W, int mask_dtype) {
    if (V == 0) return e ? SC_OK : fail(SC_ERR_INVALID, "null engine");
    int rc = check_view_args(e, K, R, t, masks_dev, H, W);
    if (rc) return rc;
    if (V < 0) return fail(SC_ERR_INVALID, "negative view count");
    rc = check_dtype(e, mask_dtype);
    if (rc) return rc;
    rc = use_device(e);
    if (rc) return rc;
    rc = materialize_deferred(e);
    if (rc) return rc;
    size_t es = elem_size(mask_dtype);
    int64_t row = (int64_t)W * (int64_t)es, view = row * H;
    if (e->mode == SC_MODE_CARVE) {
        if (e->pack_ride && e->views_per_launch == 0 && e->pending.empty() && V >= kMinFusedViews &&
            V <= kPackOrderMax && V < e->max_pending && pack16_eligible(masks_dev, W, mask_dtype, row, view)) {
            // the whole batch will be one fused launch: its packing waits for the flush, which knows
            // the order of the views (see flush)
            e->deferred.on = true;
            e->deferred.raw = masks_dev;
            e->deferred.V = V; e->deferred.H = H; e->deferred.W = W; e->deferred.dtype = mask_dtype;
            e->deferred.row_stride = row; e->deferred.view_stride = view;
            for (int q = 0; q < V; ++q) {
                ViewDesc d;
                fill_desc(e, d, K + 4 * q, R + 9 * q, t + 3 * q, nullptr, H, W, nullptr);
                e->pending.push_back(d);
            }
            return SC_OK;
        }
        // one pack launch for the whole batch, then carve launches per views_per_launch
        rc = enqueue_pack(e, V, K, R, t, masks_dev, H, W, mask_dtype, row, view);
    } else if (mask_dtype == SC_MASK_U8_LUT) {
        rc = enqueue_tiles(e, kFormU8Strips, V, K, R, t, masks_dev, H, W, row, view);
    } else if (e->avg_tile_f32) {
        rc = enqueue_tiles(e, kFormF32Tiles, V, K, R, t, masks_dev, H, W, row, view);
    } else {
        for (int q = 0; q < V; ++q) {
            ViewDesc d;
            fill_desc(e, d, K + 4 * q, R + 9 * q, t + 3 * q, static_cast<const char *>(masks_dev) + (int64_t)q * view, H, W);
            e->pending.push_back(d);
            rc = after_enqueue(e);
            if (rc) return rc;
        }
        return SC_OK;
    }
    return rc ? rc : after_enqueue(e);
}

int sc_average_labels(sc_engine *const *engines, int L, int V, const float *K, const float *R, const float *t,
                      const void *const *masks_dev, int H, int W) {
    if (!engines || !masks_dev || L < 1) return fail(SC_ERR_INVALID, "bad label set");
    for (int l = 0; l < L; ++l) {
        int rc = check_view_args(engines[l], K, R, t, masks_dev[l], H, W);
        if (rc) return rc;
        rc = check_dtype(engines[l], SC_MASK_U8_LUT);
        if (rc) return rc;
    }
    if (V < 0) return fail(SC_ERR_INVALID, "negative view count");
    if (V == 0) return SC_OK;
    sc_engine *e0 = engines[0];
    const int64_t row = W, view = (int64_t)W * H;
    // one launch needs: labels in groups of 2 .. 4 on one device, one grid, the same freshness, nothing pending,
    // the brick form's conditions (flush), whole 16-pixel rows; anything else goes label by label
    // (up to 4 labels: measured on a 6-label segmentation -- groups of 4 + 2, 3 + 3 or 2 + 2 + 2 -- the shared
    // launches took 16.5-17.4 ms where six launches of their own take 14.3: the labels' footprints are mixed in
    // different places, so the union of the (brick, view) pairs to project is nearly their sum, and every label
    // is dragged through every pair.  3 labels: 3.6 ms against 4.5.)
    const AvgPlan ap = avg_plan(e0);
    const uint32_t abys = ap.bricks_y, abzs = ap.bricks_z, anb = ap.nbricks;
    bool fused = L >= 2 && L <= kMaxLabels && V > 1 && e0->avg_brick && ap.fits && (W % 16) == 0 && V <= 4096;
    for (int l = 0; l < L && fused; ++l) {
        const sc_engine *e = engines[l];
        fused = e->device == e0->device && e->nx == e0->nx && e->ny == e0->ny && e->nz == e0->nz && e->i0 == e0->i0 &&
                e->istride == e0->istride && e->planes == e0->planes && e->vs == e0->vs &&
                memcmp(e->origin, e0->origin, sizeof e->origin) == 0 && e->fresh == e0->fresh && e->pending.empty() &&
                !e->deferred.on && e->avg_brick && (reinterpret_cast<uintptr_t>(masks_dev[l]) % 16) == 0;
        for (int m = 0; m < l && fused; ++m) fused = engines[m] != e;
    }
    if (!fused) {
        for (int l = 0; l < L; ++l) {
            int rc = sc_process_views_device(engines[l], V, K, R, t, masks_dev[l], H, W, SC_MASK_U8_LUT);
            if (rc) return rc;
            rc = sc_flush(engines[l]);
            if (rc) return rc;
        }
        return SC_OK;
    }
    int rc = use_device(e0);
    if (rc) return rc;
    // everything of this call runs on the first engine's stream, behind what the others have on theirs; their
    // streams take up again behind it
    hipStream_t main = e0->stream;
    std::vector<hipStream_t> own((size_t)L);
    for (int l = 0; l < L; ++l) own[(size_t)l] = engines[l]->stream;
    // the ordering first, for every engine; the `stream` fields are switched only once all of it has succeeded, and
    // whatever way this function is left they go back to the engines' own (an engine must never keep another's)
    for (int l = 1; l < L; ++l) {
        if (own[(size_t)l] == main) continue;
        rc = order_streams(own[(size_t)l], main, "stream ordering failed");
        if (rc) return rc;
    }
    struct StreamGuard {
        sc_engine *const *eng;
        const std::vector<hipStream_t> &own;
        int n;
        ~StreamGuard() { for (int l = 0; l < n; ++l) eng[l]->stream = own[(size_t)l]; }
    } guard{engines, own, L};
    for (int l = 0; l < L; ++l) engines[l]->stream = main;
    const GridDesc g = grid_desc(e0);
    const size_t need = (size_t)anb * (size_t)V;
    const ViewDesc *vd[64];
    rc = SC_OK;
    for (int l = 0; l < L && rc == SC_OK; ++l) {
        sc_engine *e = engines[l];
        rc = enqueue_tiles(e, kFormU8Strips, V, K, R, t, masks_dev[l], H, W, row, view);
        if (rc) break;
        if (!brick_view(e, e->pending[0])) { rc = fail(SC_ERR_STATE, "no uniformity flags"); break; }
        const ViewDesc *pin;
        rc = stage_descriptors(e, (size_t)V, &vd[l < 64 ? l : 0], &pin);
        if (rc) break;
        if (hipMemcpyAsync(const_cast<ViewDesc *>(vd[l < 64 ? l : 0]), pin, (size_t)V * sizeof(ViewDesc), hipMemcpyHostToDevice, main) !=
            hipSuccess) { rc = fail(SC_ERR_DEVICE, "descriptor copy failed"); break; }
        rc = grow_verdicts(e, need, false);
        if (rc) break;
    }
    if (rc == SC_OK && L > 64) rc = fail(SC_ERR_INVALID, "more than 64 labels");
    for (int l0 = 0; l0 < L && rc == SC_OK; l0 += kMaxLabels) {
        const int n = std::min(kMaxLabels, L - l0);
        if (n == 1) {  // a label left over: its own launches (on `main`: the engine's stream for now)
            rc = launch_average_bricks(engines[l0], g, vd[l0], V, nullptr, false);
            continue;
        }
        MultiArgs a;
        memset(&a, 0, sizeof a);
        for (int q = 0; q < n; ++q) {
            sc_engine *e = engines[l0 + q];
            a.values[q] = static_cast<float *>(e->state.get());
            a.views[q] = vd[l0 + q];
            a.verd[q] = e->verd;
            a.lut[q] = e->lut_dev;
            a.init[q] = e->default_value;
        }
#define LAUNCH_MULTI(N)                                                                                              \
    do {                                                                                                             \
        hipLaunchKernelGGL((avg_flags_multi_kernel<N>), dim3((anb + kBlock - 1) / kBlock, (uint32_t)V), dim3(kBlock), 0, main, a, g, \
                           V, abys, abzs, anb, static_cast<uint8_t *const *>(nullptr));                              \
        if (e0->fresh) hipLaunchKernelGGL((average_multi_kernel<N, true>), dim3(anb), dim3(kBlock), 0, main, a, g, V, abys, abzs); \
        else hipLaunchKernelGGL((average_multi_kernel<N, false>), dim3(anb), dim3(kBlock), 0, main, a, g, V, abys, abzs);          \
    } while (0)
        if (n == 2) LAUNCH_MULTI(2);
#if SC_MAXLABELS >= 3
        else if (n == 3) LAUNCH_MULTI(3);
#endif
#if SC_MAXLABELS >= 4
        else LAUNCH_MULTI(4);
#endif
#undef LAUNCH_MULTI
    }
    if (rc == SC_OK && hipGetLastError() != hipSuccess) rc = fail(SC_ERR_DEVICE, "multi-label launch failed");
    // the other engines' own streams wait for the first one's
    if (rc == SC_OK) {
        Event ev;  // (released once the waits have been satisfied)
        hipError_t he = hipEventCreateWithFlags(ev.out(), hipEventDisableTiming);
        if (he == hipSuccess) he = hipEventRecord(ev, main);
        for (int l = 1; l < L && he == hipSuccess; ++l)
            if (own[(size_t)l] != main) he = hipStreamWaitEvent(own[(size_t)l], ev, 0);
        if (he != hipSuccess) rc = fail(SC_ERR_DEVICE, "stream ordering failed: %s", hipGetErrorString(he));
    }
    for (int l = 0; l < L; ++l) {
        sc_engine *e = engines[l];
        e->pending.clear();
        if (rc == SC_OK) e->fresh = false;
        arena_reset(e);  // (on the first engine's stream, which every later use of this engine's arena is behind)
    }
    if (rc == SC_OK) g_avg_labels_fused.fetch_add(1, std::memory_order_relaxed);
    return rc;  // (the guard hands the engines their own streams back)
}

int64_t sc_average_labels_fused_count(void) { return g_avg_labels_fused.load(std::memory_order_relaxed); }

}  // extern "C"
