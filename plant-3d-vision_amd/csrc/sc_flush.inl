// Part of spacecarve.hip (included there, behind sc_engine.h): what a batch of pending views becomes on the stream --
// FusedPlan / flush() and the launches it dispatches to (the seven kernels of a fused carve, the streaming kernel, the
// averaging forms), the stream pool, the device half of an engine's set-up and create().

namespace {

static_assert(kListBlocks % 8 == 0 && kBrickWalkers % 8 == 0, "the dense stage's walkers come in whole groups of 8 XCDs");

// What a fused carve of `nv` views will look like (see flush): decided before anything is launched,
// because a deferred batch is packed according to it.
struct FusedPlan {
    int ndense, nstage1, s1, flag_views;
    bool compact, brick;
    uint32_t bys, bzs, nbricks, nstrips;
};

FusedPlan fused_plan(const sc_engine *e, size_t nv, bool has_occ) {
    FusedPlan p{};
    p.ndense = (int)e->dense_views;
    p.nstage1 = (int)e->stage1_views;
    p.compact = e->compact && nv >= (size_t)kMinFusedViews && nv > (size_t)p.ndense &&
                (uint64_t)e->npitch < 0x80000000ull;
    p.bys = (uint32_t)((e->ny + kBrickY - 1) / kBrickY);
    p.bzs = (uint32_t)((e->nz + kBrickZ - 1) / kBrickZ);
    p.brick = (nv > 1 || e->view_brick) && e->brick && p.bzs <= 64 && (uint64_t)e->npitch < 0x80000000ull &&
              (uint64_t)e->planes * p.bys * p.bzs < 0x40000000ull && has_occ;  // brick ids carry two flag bits in the fill list
    p.nbricks = p.brick ? (uint32_t)((uint64_t)e->planes * p.bys * p.bzs) : 0u;
    p.flag_views = (int)nv;  // every view of the batch may veto a brick, not only the dense stage's
    if (e->flag_views > 0 && e->flag_views < (int64_t)p.flag_views) p.flag_views = (int)e->flag_views;
    p.s1 = (int)std::min<size_t>(nv, (size_t)p.ndense + (size_t)p.nstage1);
    // the -1 fill of the bricks found empty: with survivor stages it rides along with them (carve_list_kernel's store
    // blocks), without them it is the light dense kernel's
    p.nstrips = p.brick ? (uint32_t)((uint64_t)e->planes * p.bys) : 0u;
    return p;
}

// How a deferred device batch was packed (pack_deferred): the views [packed_ahead, nv) are left to riders beside the
// dense stage (`blocks` of them, 0: none).
struct Ride {
    PackJob job;
    uint32_t blocks;
    int packed_ahead;
    bool ordered;  // the pending views are in the order they will be applied already
};

// The REACH RECTANGLE of a view (ViewDesc::reach): the 32x32 tiles of its picture that a voxel of this engine --
// planes i0 + k istride, every column, every voxel -- or a verdict about a brick or a unit of it can look at.  Readers
// take whole bricks, those that stick out of the grid at its far y / z faces included, so the box is the engine's
// planes x whole bricks.  Under a certified view with every corner well in front of the camera the image of that
// convex box is the hull of its eight corners' images (DESIGN_APPENDIX.md 4b), worked out here in double precision
// from the kernels' own float coordinates.  A reader's widened pixel box (rect_box) lies within twice its slack of
// the exact image, and the slack grows with the box: the hull is widened by the slack mu of the WHOLE box plus one
// whole tile, which covers 2 mu as long as mu <= 32 -- beyond that, for an uncertified view, a corner not in front or
// anything not finite, the rectangle is the whole picture (0).  An image that misses the picture: the empty rectangle.
uint64_t reach_rect(const sc_engine *e, const ViewDesc &d) {
    const int64_t tiles_x = (d.W + kTile - 1) / kTile, tiles_y = (d.H + kTile - 1) / kTile;
    if (d.safe == 0 || tiles_x > 0xffff || tiles_y > 0xffff) return 0;
    const int64_t last[3] = {e->i0 + (e->planes - 1) * e->istride, (e->ny + kBrickY - 1) / kBrickY * kBrickY - 1,
                             (e->nz + kBrickZ - 1) / kBrickZ * kBrickZ - 1};
    const int64_t first[3] = {e->i0, 0, 0};
    double c[3][2];  // the box's extremes per axis, as the kernels compute a coordinate: origin + (float)index * voxel_size
    for (int a = 0; a < 3; ++a) {
        c[a][0] = (double)(e->origin[a] + (float)first[a] * e->vs);
        c[a][1] = (double)(e->origin[a] + (float)last[a] * e->vs);
    }
    double err[3], pzmin = INFINITY, umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, qxm = 0.0, qym = 0.0;
    for (int r = 0; r < 3; ++r) {  // rows of R: x, y, depth
        err[r] = std::fabs((double)d.t[r]);
        for (int a = 0; a < 3; ++a) err[r] += std::fabs((double)d.R[3 * r + a]) * std::max(std::fabs(c[a][0]), std::fabs(c[a][1]));
        err[r] *= 0x1p-19;
    }
    for (int q = 0; q < 8; ++q) {
        const double X[3] = {c[0][q & 1], c[1][(q >> 1) & 1], c[2][(q >> 2) & 1]};
        double p[3];
        for (int r = 0; r < 3; ++r) p[r] = (double)d.R[3 * r] * X[0] + (double)d.R[3 * r + 1] * X[1] + (double)d.R[3 * r + 2] * X[2] + (double)d.t[r];
        if (!(p[2] > 8.0 * err[2]) || !(p[2] > 0x1p-10)) return 0;  // (also NaN)
        const double qx = p[0] / p[2], qy = p[1] / p[2];
        const double u = qx * (double)d.K[0] + (double)d.K[2], v = qy * (double)d.K[1] + (double)d.K[3];
        if (!std::isfinite(u) || !std::isfinite(v)) return 0;
        pzmin = std::min(pzmin, p[2]);
        umin = std::min(umin, u); umax = std::max(umax, u);
        vmin = std::min(vmin, v); vmax = std::max(vmax, v);
        qxm = std::max(qxm, std::fabs(qx)); qym = std::max(qym, std::fabs(qy));
    }
    // rect_box's slack (sc_verdicts.h), with the box's extremes
    const double inv = 2.0 / pzmin;
    const double mu = 2.0 + std::fabs((double)d.K[0]) * (err[0] + qxm * err[2]) * inv +
                      (std::fabs((double)d.K[0]) * qxm + std::fabs((double)d.K[2]) + std::max(std::fabs(umin), std::fabs(umax))) * 0x1p-20;
    const double mv = 2.0 + std::fabs((double)d.K[1]) * (err[1] + qym * err[2]) * inv +
                      (std::fabs((double)d.K[1]) * qym + std::fabs((double)d.K[3]) + std::max(std::fabs(vmin), std::fabs(vmax))) * 0x1p-20;
    if (!(mu <= 32.0 && mv <= 32.0)) return 0;
    const double ulo = umin - mu - 32.0, uhi = umax + mu + 32.0, vlo = vmin - mv - 32.0, vhi = vmax + mv + 32.0;
    if (uhi < 0.0 || vhi < 0.0 || ulo > (double)d.W - 1.0 || vlo > (double)d.H - 1.0) return 1ull | (1ull << 16) | (1ull << 32) | (1ull << 48);  // empty
    const uint64_t tx0 = (uint64_t)std::floor(std::max(ulo, 0.0) / 32.0), tx1 = (uint64_t)std::floor(std::min(uhi, (double)d.W - 1.0) / 32.0) + 1;
    const uint64_t ty0 = (uint64_t)std::floor(std::max(vlo, 0.0) / 32.0), ty1 = (uint64_t)std::floor(std::min(vhi, (double)d.H - 1.0) / 32.0) + 1;
    return tx0 | (tx1 << 16) | (ty0 << 32) | (ty1 << 48);
}

// A device batch whose packing was deferred is packed here, in the order its views will be applied: the views the
// flags kernel, the dense stage and the first survivor stage need go ahead, the others ride beside the dense stage
// (brick form).  Any other shape of launch packs the whole batch first, in the order given.
int pack_deferred(sc_engine *e, size_t nv, Ride *r) {
    memset(r, 0, sizeof *r);
    r->packed_ahead = (int)nv;
    for (int q = 0; q < 4; ++q) e->pack_cnt[q] = 0;  // sc_pack_counts speaks of the last flushed batch
    e->pack_cnt_riders = false;
    if (!e->deferred.on) return SC_OK;
    const bool whole = nv == e->pending.size() && nv == (size_t)e->deferred.V && e->mode == SC_MODE_CARVE && nv > 1;
    if (!whole) return materialize_deferred(e);
    int rc = step_begin(e);
    if (rc) return rc;
    std::vector<uint32_t> perm;
    if (e->view_order == 1) order_views(e->pending, &perm);
    else { perm.resize(nv); for (size_t q = 0; q < nv; ++q) perm[q] = (uint32_t)q; }
    r->ordered = true;
    PackJob pj;
    rc = deferred_job(e, &pj);
    if (rc) return rc;
    e->deferred.on = false;
    pj.use_order = 1;
    for (size_t q = 0; q < nv; ++q) pj.order[q] = (uint16_t)perm[q];
    const FusedPlan fp = fused_plan(e, nv, true);
    int ahead = (int)nv;
    // (riders only where the list stages' store blocks do all of the fill: with riders the flags kernel leaves FULL
    // candidates open until the confirm kernel -- behind the dense kernel -- and only the list stages come after that)
    if (e->pack_ride && fp.brick && fp.compact) ahead = std::min<int>((int)nv, std::max(fp.flag_views, fp.s1));
    pj.slot0 = 0;
    pj.nslots = ahead;
    // every view's reach rectangle: in its descriptor, and in the job for the packers (ahead and riders alike)
    pj.reach_on = e->pack_reach ? 1 : 0;
    const int64_t view_tiles = (int64_t)pj.tiles_x * pj.tiles_y;
    for (size_t q = 0; q < nv; ++q) {
        ViewDesc &d = e->pending[q];
        // (a slot the job has no room for is packed whole, and its descriptor says so: field and arena agree)
        d.reach = (e->pack_reach && q < (size_t)kReachViews) ? reach_rect(e, d) : 0;
        if (q < (size_t)kReachViews)
            for (int w = 0; w < 4; ++w) pj.reach[q][w] = (uint16_t)(d.reach >> (16 * w));
        if ((int)q < ahead) {
            const TileRect rc = rect_unpack(d.reach, pj.tiles_x, pj.tiles_y);
            e->pack_cnt[0] += (int64_t)std::max(0, rc.tx1 - rc.tx0) * std::max(0, rc.ty1 - rc.ty0);
            e->pack_cnt[1] += view_tiles;
        } else {
            e->pack_cnt[3] += view_tiles;
        }
    }
    LaunchTimer ltp{e, SC_KERNEL_PACK};
    rc = ltp.begin();
    if (rc) return rc;
    rc = launch_pack16(e, pj);
    if (rc) return rc;
    rc = ltp.end();
    if (rc) return rc;
    if (ahead < (int)nv) {
        r->job = pj;
        r->job.slot0 = ahead;
        r->job.nslots = (int)nv - ahead;
        const int64_t rb = pack16_blocks(e, r->job);
        if (rb > 0x3fffffffLL) return fail(SC_ERR_INVALID, "mask batch too large");
        r->blocks = (uint32_t)rb;
        r->packed_ahead = ahead;
        e->pack_cnt_riders = true;  // pack_cnt[2] is on the device (ListCtl::rider_tiles)
    }
    return SC_OK;
}

// The first `nv` pending descriptors into the engine's descriptor ring: *pin (page-locked) holds them, *dev is where
// they go on the device -- by a copy on the stream, or through the flags kernel's arguments (brick form).  Slots are
// reused only after a wrap, which waits for the stream.
int stage_descriptors(sc_engine *e, size_t nv, const ViewDesc **dev, const ViewDesc **pin) {
    if (nv > e->views_cap || e->views_head + nv > e->views_cap) {
        HIP_TRY(schost::wait_stream(e->stream));
        e->views_head = 0;
    }
    if (nv > e->views_cap) {
        const size_t cap = std::max<size_t>(nv * 8, 4096);  // (a wrap every 56 batches of 72 views; 1024 until round 4)
        auto ring = [&] {
            const hipError_t he = sc_dev_malloc(e->views_dev.out(), cap * sizeof(ViewDesc));
            return he != hipSuccess ? he : sc_pin_malloc(e->views_pin.out(), cap * sizeof(ViewDesc), hipHostMallocDefault);
        };
        HIP_TRY(scown::grow(e->views_cap, cap, [] { return hipSuccess; }, ring, e->views_dev, e->views_pin));  // (waited above)
    }
    memcpy(e->views_pin + e->views_head, e->pending.data(), nv * sizeof(ViewDesc));
    *pin = e->views_pin + e->views_head;
    *dev = e->views_dev + e->views_head;
    e->views_head += nv;
    return SC_OK;
}

// A fused carve of `nv` views (or of one view in brick form), as fused_plan() shapes it; what its launches share.
struct CarveBatch {
    size_t nv;
    FusedPlan fp;
    const ViewDesc *vd, *vpin;
    int32_t *st;
    int32_t init;
    Append ap;
    int dense_views;
    bool bulk_on, desc_by_flags;
    uint32_t parity, cand_per, spec_strips;
};

// Brick form: the flags kernel, then the dense kernel -- walkers on the live list and packing riders (with survivor
// stages), or walkers and fillers (the light kernel, without).  `lt` times the dense kernel alone.
int launch_dense_bricks(sc_engine *e, const GridDesc &g, const CarveBatch &b, const Ride &ride, LaunchTimer &lt) {
    const FusedPlan &fp = b.fp;
    const dim3 block(kBlock);
    const uint32_t nbricks = fp.nbricks, bys = fp.bys, bzs = fp.bzs;
    // live-list walkers (whole groups of 8 XCDs), then packing riders; with riders the walkers leave wavefront slots free
    // for them
    const uint32_t nwalkers = ride.blocks ? kBrickWalkers : kListBlocks;
    if (!e->dead) {
        HIP_TRY(sc_dev_malloc(e->dead.out(), (size_t)nbricks));
        e->dead_clean = false;
    }
    const int dead_stale = e->dead_clean ? 0 : 1;  // the flags kernel rewrites them all
    e->dead_clean = true;
    // unit verdicts (cell level) by the views packed ahead, inside the dense stage
    int nverd = 0;
    const uint32_t verd_max_live = e->unit_cull == 2 ? 0xffffffffu : (uint32_t)(nbricks / 2);
    const uint32_t bulk_min_live = (uint32_t)((uint64_t)nbricks * (uint64_t)e->bulk_live / 16u);
    if (fp.compact && e->unit_cull) {
        nverd = std::min(ride.packed_ahead, 16);
        for (int q = 0; q < nverd; ++q)
            if (e->pending[(size_t)q].cmask == nullptr) nverd = 0;
    }
    LaunchTimer ltf{e, SC_KERNEL_FLAGS};
    int rc = ltf.begin();
    if (rc) return rc;
    FlagViews own{};
    DescCopy dc{nullptr, nullptr, 0u};
    if (b.desc_by_flags) {
        for (int q = 0; q < fp.flag_views; ++q) own.v[q] = e->pending[(size_t)q];
        dc = DescCopy{reinterpret_cast<const uint32_t *>(b.vpin), reinterpret_cast<uint32_t *>(const_cast<ViewDesc *>(b.vd)),
                      (uint32_t)(b.nv * sizeof(ViewDesc) / 4)};
    }
    SpecFill sf{nullptr, 0u, 0u};
    if (b.spec_strips > 0) {
        // strip s starts at column (s / bys) * ny + (s % bys) * 16; the columns are contiguous rows of nzp labels
        const uint64_t cols = (uint64_t)(b.spec_strips / bys) * (uint64_t)e->ny + (uint64_t)(b.spec_strips % bys) * kBrickY;
        sf = SpecFill{b.st, cols * (uint64_t)e->nzp * 4u, kSpecBlocks};
    }
    const bool compact = fp.compact;
    hipLaunchKernelGGL(brick_flags_kernel, dim3(sf.nblocks + (nbricks + 63u) / 64u), dim3(64 * kFlagWaves), 0,
                       e->stream, g, b.desc_by_flags ? static_cast<const ViewDesc *>(nullptr) : b.vd,
                       fp.flag_views, bys, bzs, nbricks, e->flags, e->live, e->ctl, own, dc,
                       b.desc_by_flags ? b.vpin : b.vd, e->full_bricks ? ride.packed_ahead : 0, (int)b.nv, e->dead,
                       dead_stale, b.parity, compact ? static_cast<uint32_t *>(nullptr) : e->fill_list, sf,
                       compact ? e->fill_list : static_cast<uint32_t *>(nullptr), b.cand_per);  // (the room of the fill list holds the candidate list when nothing fills from a list)
    e->last_parity = b.parity;
    rc = ltf.end();
    if (rc) return rc;
    rc = lt.begin();  // SC_KERNEL_CARVE times the dense kernel alone
    if (rc) return rc;
    if (!compact) {
        // no survivor stages: walkers on the live list, fillers on the fill list
        const dim3 lgrid(nwalkers + kStoreBlocks);
        hipLaunchKernelGGL(e->fresh ? carve_brick_light_kernel<true> : carve_brick_light_kernel<false>, lgrid, block, 0, e->stream,
                           b.st, g, b.vd, b.dense_views, b.init, bys, bzs, e->live, e->fill_list, e->ctl, nwalkers, b.parity);
        return SC_OK;
    }
    // (every dense view certified by the host: the instance without the general projection path)
    // (a thinned-out unit may take one more pair of the views packed ahead: brick_voxels)
    const int nextra = std::max(0, std::min(2, ride.packed_ahead - b.dense_views));
    bool dense_safe = e->safe_kernels != 0;
    for (int q = 0; q < b.dense_views + nextra && dense_safe; ++q) dense_safe = e->pending[(size_t)q].safe != 0;
    auto *dense = e->fresh ? (dense_safe ? carve_brick_kernel<true, true> : carve_brick_kernel<true, false>)
                           : (dense_safe ? carve_brick_kernel<false, true> : carve_brick_kernel<false, false>);
    hipLaunchKernelGGL(dense, dim3(nwalkers + ride.blocks), block, 0, e->stream, b.st, g, b.vd, b.dense_views, b.init, b.ap, bys, bzs,
                       e->flags, e->live, e->ctl, nwalkers, ride.job, pack_form(e, ride.job), b.parity, nverd, verd_max_live,
                       bulk_min_live, nextra);
    return SC_OK;
}

// The survivor stages behind the dense stage: the confirm kernel (with riders), the special kernel, the first list
// stage and the final one.  In brick form the list stages' store blocks do the -1 fill of the bricks found empty.
int launch_list_stages(sc_engine *e, const GridDesc &g, const CarveBatch &b, const Ride &ride) {
    const FusedPlan &fp = b.fp;
    const size_t nv = b.nv;
    const int ndense = fp.ndense, s1 = fp.s1;
    const uint32_t bys = fp.bys, bzs = fp.bzs, nbricks = fp.nbricks, nstrips = fp.nstrips, spec_strips = b.spec_strips;
    const ViewDesc *vd = b.vd;
    int32_t *st = b.st;
    const int32_t init = b.init;
    const dim3 block(kBlock);
    uint32_t *l0 = e->lists, *l1 = e->lists + (size_t)kSub * e->subcap;
    LaunchTimer lt2{e, SC_KERNEL_LIST};
    int rc = lt2.begin();
    if (rc) return rc;
    // open FULL candidates exist only when packing rode beside the dense stage
    if (ride.blocks) {
        e->sparse_late = true;
        // the riders have packed the rest of the masks: open FULL candidates get their answer
        // (a block per 64 entries of the candidate list, a persistent grid of at most 4096; without candidates
        // every block leaves after eight scalar loads)
        const uint32_t nconfirm = std::min<uint32_t>((nbricks + 63u) / 64u, 4096u);
        // (a candidate that fails takes the bulk units' road when the batch has a bulk list: UnitRoad)
        const UnitRoad road{(b.bulk_on && e->late_road) ? st : nullptr, init, e->fresh ? 1 : 0, nbricks};
        hipLaunchKernelGGL(brick_confirm_kernel, dim3(nconfirm), dim3(64 * kConfirmWaves), 0, e->stream, g, vd,
                           ride.packed_ahead, (int)nv, bys, bzs, e->flags, e->fill_list, b.cand_per, e->late, e->ctl, b.parity, road);
    }
    // Too few bulk units for their verdicts are taken by the first survivor stage as they are (UnitSpill); a
    // batch with a single (final) list stage has no such stage: its units are always asked
    const uint32_t unit_floor = (size_t)s1 >= nv ? 0u : (uint32_t)e->bulk_floor;
    {
        // bulk units, late bricks, the dense fallback, the next batch's counters: one launch, always there
        // (what it finds to do is decided on the device)
        SpecialJob sj;
        memset(&sj, 0, sizeof sj);
        if (b.bulk_on)
            sj.uj = UnitJob{e->bulk, e->bulkcap, e->items, e->itemcap, vd, (int32_t)nv, ndense, bys, bzs, st,
                            e->lists, e->subcap, kItemBias, unit_floor};
        sj.lb = LateBricks{ride.blocks ? e->late : nullptr, nbricks, vd, e->flags, (int32_t)nv, init, e->fresh ? 1 : 0, bys, bzs};
        sj.next = e->ctl2[e->ctl_idx ^ 1];
        sj.rest = vd + ndense;
        sj.nrest = (int32_t)nv - ndense;
        sj.flags = fp.brick ? e->flags : nullptr;
        sj.bricks_y = bys;
        sj.bricks_z = bzs;
        hipLaunchKernelGGL(carve_special_kernel, dim3(kUnitBlocks), dim3(64 * kFlagWaves), 0, e->stream, st, g, e->ctl, sj);
        e->ctl_clean[e->ctl_idx ^ 1] = true;
    }
    // Brick form: the final stage runs kFinalListBlocks persistent list blocks (they leave wavefront slots free) and
    // kStoreBlocks store blocks walking the strips behind them; the first stage, when there is one, takes a share of the
    // fill as well (it waits on memory).  The strips a fresh volume filled ahead come first, then the first stage's share.
    CullStores cs{nullptr, 0u, 0u, 0u, 0u, 0, 0, 0u, 0, 0u}, cs1 = cs;
    dim3 grid1(kListBlocks), fgrid(kListBlocks);
    if (fp.brick) {
        uint32_t mid = spec_strips;
        if ((size_t)s1 < nv) {
            mid += (uint32_t)((uint64_t)(nstrips - spec_strips) * kStage1StoreShare / 16u);
            const uint32_t f1 = std::min(kStoreBlocks, mid - spec_strips);
            cs1 = CullStores{e->flags, bys, bzs, mid, spec_strips, init == 0 ? 1 : init, e->fresh ? 1 : 0, f1, init, 0u};
            grid1 = dim3(kStage1ListBlocks + f1);
        }
        // (the final stage also walks the strips filled ahead, for their FULL / UNTOUCHED bricks)
        const uint32_t ff = std::min(kStoreBlocks, nstrips - mid + spec_strips);
        cs = CullStores{e->flags, bys, bzs, nstrips, mid, init == 0 ? 1 : init, e->fresh ? 1 : 0, ff, init, spec_strips};
        fgrid = dim3(kFinalListBlocks + ff);
    }
    // every view of the batch certified by the host (certify_view: any real rig): the instances without the general path
    bool all_safe = e->safe_kernels != 0;
    for (size_t q = 0; q < nv && all_safe; ++q) all_safe = e->pending[q].safe != 0;
    // (two survivors per lane in both stages: the instances with one and with four were retired with their
    // knobs in round 6, and so was the optional second stage)
    auto *stage1_kernel = all_safe ? carve_list_kernel<false, 2, true> : carve_list_kernel<false, 2>;
    auto *final_kernel = all_safe ? carve_list_kernel<true, 2, true> : carve_list_kernel<true, 2>;
    // stage 1 (l0 -> l1), final stage on what is left
    uint32_t *nolist = nullptr;
    // the final stage also takes the work items of the bulk units
    const UnitItems noitems{nullptr, 0u, nullptr, 0u, 0u}, ui{b.bulk_on ? e->items : nullptr, e->itemcap, vd, bys, bzs};
    // ... the first one the bulk units of a batch that has too few for their verdicts (decided on the device)
    const UnitSpill nospill{nullptr, 0u, 0u, 0u, 0u}, us{b.bulk_on ? e->bulk : nullptr, e->bulkcap, unit_floor, bys, bzs};
    const int vg = kViewGroup;
    if ((size_t)s1 >= nv) {
        hipLaunchKernelGGL(final_kernel, fgrid, block, 0, e->stream, st, g, vd + ndense, s1 - ndense, l0, nolist, e->ctl, 0, 0, e->subcap, vg,
                           cs, ui, nospill, s1 - ndense);
    } else {
        hipLaunchKernelGGL(stage1_kernel, grid1, block, 0, e->stream, st, g, vd + ndense, s1 - ndense, l0, l1, e->ctl, 0, 1, e->subcap, vg,
                           cs1, noitems, us, (int)nv - ndense);
        hipLaunchKernelGGL(final_kernel, fgrid, block, 0, e->stream, st, g, vd + s1, (int)nv - s1, l1, nolist, e->ctl, 1, 1, e->subcap, vg,
                           cs, ui, nospill, (int)nv - s1);
    }
    HIP_TRY(hipGetLastError());
    return lt2.end();
}

// The fused carve of a batch, or of one view in brick form: dense for the first `ndense` views (brick form: behind the
// flags kernel's verdicts), then -- survivor compaction -- the list stages.
int carve_batch(sc_engine *e, size_t nv, const GridDesc &g, const ViewDesc *vd, const ViewDesc *vpin, const Ride &ride) {
    CarveBatch b{nv, fused_plan(e, nv, e->pending[0].occ != nullptr), vd, vpin, static_cast<int32_t *>(e->state.get()), init_bits_i32(e)};
    const FusedPlan &fp = b.fp;
    const bool compact = fp.compact, brick = fp.brick;
    // what sc_values_sparse may take from this launch's verdict bytes and lists (sc_sparse.h)
    e->sparse_exact = brick && e->fresh;
    e->sparse_late = false;
    b.ap = Append{nullptr, nullptr, 0u, 0u, nullptr, 0u, 0u};
    b.dense_views = (int)nv;
    // strips set to -1 ahead of the verdicts, by fill blocks in front of the flags kernel's own (SpecFill): a fresh
    // volume, whose fill is otherwise all the list stages' (so that everything behind the flags kernel that writes labels
    // comes later on the stream)
    if (brick && compact && e->fresh) b.spec_strips = (uint32_t)((uint64_t)fp.nstrips * kSpecShare / 16u);
    // the descriptors reach the device array either by a copy on the stream, or -- brick form -- through the flags
    // kernel, which gets its own in its arguments
    b.desc_by_flags = brick && fp.flag_views <= kFlagWaves;
    if (!b.desc_by_flags)
        HIP_TRY(hipMemcpyAsync(const_cast<ViewDesc *>(vd), vpin, nv * sizeof(ViewDesc), hipMemcpyHostToDevice, e->stream));
    int rc;
    if (compact || brick) {
        rc = ensure_ctl(e);
        if (rc) return rc;
        // list counters, overflow flag, live-brick count: this batch takes the block the previous
        // batch's final stage left zeroed (a memset only if there was no such stage)
        if (compact) {
            e->ctl_idx ^= 1;
            e->ctl = e->ctl2[e->ctl_idx];
            if (!e->ctl_clean[e->ctl_idx]) HIP_TRY(hipMemsetAsync(e->ctl, 0, sizeof(ListCtl), e->stream));
        }
        // (a launch without survivor stages keeps the block: its two counters alternate, see ListCtl)
        e->ctl_clean[e->ctl_idx] = false;
    }
    b.parity = (uint32_t)(e->flag_launches & 1u);
    // blocks of the flags kernel per sub-list of the candidate list (ListCtl::ncand): sub-list s holds the candidates of
    // blocks [s per, (s + 1) per) at cands + s per 64 -- at most the bricks of those blocks, so the lists fit in nbricks words
    b.cand_per = std::max<uint32_t>(1u, (uint32_t)(((fp.nbricks + 63u) / 64u + kCandSub - 1) / kCandSub));
    if (brick) ++e->flag_launches;
    if (compact) {
        rc = ensure_lists(e);
        if (rc) return rc;
        b.ap.list = e->lists;
        b.ap.ctl = e->ctl;
        b.ap.subcap = e->subcap;
        b.dense_views = fp.ndense;
    }
    // bulk units: brick form with survivor stages, every view with its cell level
    b.bulk_on = compact && brick && e->bulk_min > 0 && e->bulk != nullptr && e->items != nullptr;
    if (nv > 128) b.bulk_on = false;  // the units' verdict masks cover 128 views
    for (size_t q = 0; q < nv && b.bulk_on; ++q) b.bulk_on = e->pending[q].cmask != nullptr;
    if (b.bulk_on) {
        b.ap.bulk = e->bulk;
        b.ap.bulkcap = e->bulkcap;
        b.ap.bulk_min = (uint32_t)e->bulk_min;
    }
    e->last_bulk = b.bulk_on;
    LaunchTimer lt{e, SC_KERNEL_CARVE};
    if (brick) {
        rc = launch_dense_bricks(e, g, b, ride, lt);  // (starts the timer after its flags kernel)
        if (rc) return rc;
    } else {
        rc = lt.begin();
        if (rc) return rc;
        hipLaunchKernelGGL((e->fresh ? carve_kernel<true, true> : carve_kernel<false, true>), dim3((uint32_t)((g.ngroups + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, e->stream, b.st, g, vd, b.dense_views, b.init, b.ap);
    }
    HIP_TRY(hipGetLastError());
    rc = lt.end();
    if (rc) return rc;
    return compact ? launch_list_stages(e, g, b, ride) : SC_OK;
}

// One view, not in brick form: the streaming kernel, its descriptor in the kernel arguments.
int carve_stream(sc_engine *e, const GridDesc &g) {
    e->sparse_exact = false;
    e->sparse_late = false;
    e->last_bulk = false;
    LaunchTimer lt{e, SC_KERNEL_CARVE};
    int rc = lt.begin();
    if (rc) return rc;
    // kStreamGroups groups per lane when the state is streamed through (see kernel)
    const uint32_t per_block = !e->fresh ? kBlock * kStreamGroups : kBlock;
    const dim3 grid1((uint32_t)((g.ngroups + per_block - 1) / per_block));
    hipLaunchKernelGGL((e->fresh ? carve_kernel_1<true, true> : carve_kernel_1<false, true>), grid1, dim3(kBlock), 0, e->stream,
                       static_cast<int32_t *>(e->state.get()), g, e->pending[0], init_bits_i32(e));
    HIP_TRY(hipGetLastError());
    return lt.end();
}

// The brick averaging form's verdict buffers, `need` elements each, grown behind the stream.
int grow_verdicts(sc_engine *e, size_t need, bool f32) {
    HIP_TRY(scown::grow(e->verd_cap, need, stream_idle(e), [&] { return sc_dev_malloc(e->verd.out(), need); }, e->verd));
    if (f32) HIP_TRY(scown::grow(e->verdf_cap, need, stream_idle(e), [&] { return sc_dev_malloc(e->verdf.out(), need * 4); }, e->verdf));
    return SC_OK;
}

// The brick form of an averaging launch on this engine's grid (the carve's is FusedPlan): its bricks, and whether the
// grid fits it -- element indices and brick numbers below 2^31.
struct AvgPlan {
    uint32_t bricks_y, bricks_z, nbricks;
    bool fits;
};
AvgPlan avg_plan(const sc_engine *e) {
    AvgPlan p{};
    p.bricks_y = (uint32_t)((e->ny + kBrickY - 1) / kBrickY);
    p.bricks_z = (uint32_t)((e->nz + kBrickZ - 1) / kBrickZ);
    const uint64_t n = (uint64_t)e->planes * p.bricks_y * p.bricks_z;
    p.fits = (uint64_t)e->npitch < 0x80000000ull && n < 0x80000000ull;
    p.nbricks = (uint32_t)n;
    return p;
}
// A view the brick form can take: tiled, with its uniformity flags, and bytes with their table.
bool brick_view(const sc_engine *e, const ViewDesc &d) {
    return d.occ != nullptr && ((d.form == kFormU8Strips && e->lut_dev != nullptr) || d.form == kFormF32Tiles);
}

// The brick averaging form of `nv` views (descriptors at vd, verdict buffers grown: grow_verdicts): the uniformity verdicts of every
// (brick, view), then the bricks.  `timed`: each launch under its kernel timer.
int launch_average_bricks(sc_engine *e, const GridDesc &g, const ViewDesc *vd, int nv, uint32_t *verdf, bool timed) {
    const AvgPlan ap = avg_plan(e);
    LaunchTimer ltf{e, SC_KERNEL_FLAGS}, lta{e, SC_KERNEL_AVERAGE};
    int rc = timed ? ltf.begin() : SC_OK;
    if (rc) return rc;
    hipLaunchKernelGGL(avg_flags_kernel, dim3((ap.nbricks + kBlock - 1) / kBlock, (uint32_t)nv), dim3(kBlock), 0, e->stream,
                       g, vd, nv, ap.bricks_y, ap.bricks_z, ap.nbricks, e->verd, verdf);
    rc = ltf.end();
    if (rc) return rc;
    rc = timed ? lta.begin() : SC_OK;
    if (rc) return rc;
    hipLaunchKernelGGL(e->fresh ? average_brick_kernel<true> : average_brick_kernel<false>, dim3(ap.nbricks), dim3(kBlock), 0, e->stream,
                       static_cast<float *>(e->state.get()), g, vd, nv, e->default_value, e->lut_dev, ap.bricks_y, ap.bricks_z, e->verd, verdf);
    HIP_TRY(hipGetLastError());
    return lta.end();
}

// Averaging: the brick form (uint8 masks with uniformity flags on every view of the batch, a table, a grid it fits),
// otherwise a voxel per lane and view.
int average_batch(sc_engine *e, size_t nv, const GridDesc &g, const ViewDesc *vd, const ViewDesc *vpin) {
    if (vd != nullptr)
        HIP_TRY(hipMemcpyAsync(const_cast<ViewDesc *>(vd), vpin, nv * sizeof(ViewDesc), hipMemcpyHostToDevice, e->stream));
    int rc;
    const AvgPlan ap = avg_plan(e);
    bool abrick = nv > 1 && e->avg_brick && ap.fits;
    bool any_f32 = false;
    for (size_t q = 0; q < nv && abrick; ++q) {
        abrick = brick_view(e, e->pending[q]);
        any_f32 |= e->pending[q].form == kFormF32Tiles;
    }
    if (abrick) {
        const size_t need = (size_t)ap.nbricks * nv;  // (the flat values of float32 views as well)
        rc = grow_verdicts(e, need, any_f32);
        if (rc) return rc;
        return launch_average_bricks(e, g, vd, (int)nv, any_f32 ? e->verdf.get() : nullptr, true);
    }
    LaunchTimer lt{e, SC_KERNEL_AVERAGE};
    rc = lt.begin();
    if (rc) return rc;
    float *st = static_cast<float *>(e->state.get());
    const dim3 grid((uint32_t)((g.ngroups + kBlock - 1) / kBlock)), block(kBlock);
    if (nv == 1)
        hipLaunchKernelGGL((e->fresh ? average_kernel_1<true, true> : average_kernel_1<false, true>), grid, block, 0, e->stream, st, g,
                           e->pending[0], e->default_value, e->lut_dev);
    else
        hipLaunchKernelGGL((e->fresh ? average_kernel<true, true> : average_kernel<false, true>), grid, block, 0, e->stream, st, g, vd,
                           (int)nv, e->default_value, e->lut_dev);
    HIP_TRY(hipGetLastError());
    return lt.end();
}

// Launch the first `count` pending views (count == 0: all of them).
int flush(sc_engine *e, size_t count = 0) {
    if (e->pending.empty()) return SC_OK;
    int rc = upload_hostbits(e);
    if (rc) return rc;
    const size_t nv = count ? std::min(count, e->pending.size()) : e->pending.size();
    Ride ride;
    rc = pack_deferred(e, nv, &ride);
    if (rc) return rc;
    const GridDesc g = grid_desc(e);
    if ((g.ngroups + kBlock - 1) / kBlock > 0x7fffffffULL) return fail(SC_ERR_INVALID, "grid too large for one launch");
    // (rows are whole 16-byte groups -- the pitch is a multiple of 64 voxels -- so every kernel takes its vector form)
    if (nv > 1) {
        rc = step_begin(e);
        if (rc) return rc;
    }
    // a single view in brick form goes through the same kernels as a batch: it needs its descriptor in the device
    // array too
    const bool carve = e->mode == SC_MODE_CARVE;
    const bool single_brick = nv == 1 && carve && fused_plan(e, nv, e->pending[0].occ != nullptr).brick;
    const ViewDesc *vd = nullptr, *vpin = nullptr;
    if (nv > 1 || single_brick) {
        if (!ride.ordered && carve && e->view_order == 1 && nv == e->pending.size()) order_views(e->pending);
        rc = stage_descriptors(e, nv, &vd, &vpin);
        if (rc) return rc;
    }
    if (!carve) rc = average_batch(e, nv, g, vd, vpin);
    else if (nv == 1 && !single_brick) rc = carve_stream(e, g);
    else rc = carve_batch(e, nv, g, vd, vpin, ride);
    if (rc) return rc;
    rc = step_end(e, nv > 1);
    if (rc) return rc;
    e->fresh = false;
    e->pending.erase(e->pending.begin(), e->pending.begin() + (ptrdiff_t)nv);
    if (e->pending.empty()) arena_reset(e);  // masks of launched views are dead in stream order
    return SC_OK;
}

int after_enqueue(sc_engine *e) {
    if (e->views_per_launch > 0) {
        while ((int64_t)e->pending.size() >= e->views_per_launch) {
            int rc = flush(e, (size_t)e->views_per_launch);
            if (rc) return rc;
        }
        return SC_OK;
    }
    if ((int64_t)e->pending.size() >= e->max_pending) return flush(e);
    return SC_OK;
}

int check_view_args(const sc_engine *e, const float *K, const float *R, const float *t,
                    const void *mask, int H, int W) {
    if (!e) return fail(SC_ERR_INVALID, "null engine");
    if (!K || !R || !t || !mask) return fail(SC_ERR_INVALID, "null view argument");
    // (a view's bits: below 2^32 bytes; the words of a strip of its bit tiles, H rounded up to 32: below 2^24)
    if (H <= 0 || W <= 0 || H > (1 << 24) - 32 || W > (1 << 24) || (int64_t)H * W > ((int64_t)1 << 34))
        return fail(SC_ERR_INVALID, "bad mask shape %d x %d", H, W);
    return SC_OK;
}

// Engine streams are kept between engines (round 5).  Creating a non-blocking stream is a hardware queue's worth of
// set-up in the runtime: 84-139 ms for the first one of a process and, now and then, 6-40 ms for a later one -- the
// "37 ms first batch" of a fresh engine that round 4's bench line showed on the driver's box (SC_TRACE_ALLOC=1 names the
// call).  A destroyed engine's stream (idle: sc_destroy has waited for it) goes on a short per-device list and the next
// engine on that device takes it from there; a process's first engine still pays the first creation, once.
std::mutex g_stream_mu;
std::vector<std::pair<int, hipStream_t>> g_stream_pool;  // (device, idle stream)
constexpr size_t kStreamPoolMax = 16;

// sc_prewarm: a thread that is bringing the runtime up and making the device's first stream; whoever wants a stream of
// that device waits for it (one creation, not two side by side) and finds the stream on the list
std::condition_variable g_prewarm_cv;
int g_prewarm_running[64] = {0};

hipError_t take_stream(int device, hipStream_t *out) {
    {
        std::unique_lock<std::mutex> lk(g_stream_mu);
        if (device >= 0 && device < 64) g_prewarm_cv.wait(lk, [&] { return g_prewarm_running[device] == 0; });
        for (size_t i = 0; i < g_stream_pool.size(); ++i)
            if (g_stream_pool[i].first == device) {
                *out = g_stream_pool[i].second;
                g_stream_pool.erase(g_stream_pool.begin() + (ptrdiff_t)i);
                return hipSuccess;
            }
    }
    return sctrace::timed("hipStreamCreate", __LINE__, 0, [&] { return hipStreamCreateWithFlags(out, hipStreamNonBlocking); });
}

void give_stream_back(int device, hipStream_t s) {
    {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        if (g_stream_pool.size() < kStreamPoolMax) {
            g_stream_pool.emplace_back(device, s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}

// The device half of an engine's set-up: the device is there and is a gfx950, a stream, the state.
int device_setup_body(sc_engine *e);
int device_setup(sc_engine *e) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = device_setup_body(e);
    e->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}
int device_setup_body(sc_engine *e) {
    const int device = e->device;
    // `device` is a HIP ordinal; only that device has to be a gfx950
    int ndev = 0;
    hipError_t hq = hipGetDeviceCount(&ndev);
    if (hq != hipSuccess) return fail(SC_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(hq));
    if (device < 0 || device >= ndev)
        return fail(SC_ERR_DEVICE, "device %d not available (%d HIP device(s) visible)", device, ndev);
    {
        hipDeviceProp_t prop;
        hq = sctrace::timed("hipGetDeviceProperties", __LINE__, 0, [&] { return hipGetDeviceProperties(&prop, device); });
        if (hq != hipSuccess) return fail(SC_ERR_DEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(hq));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(SC_ERR_DEVICE, "device %d is %s; this engine is built for gfx950 only", device,
                        prop.gcnArchName);
    }
    hipError_t he = sctrace::timed("hipSetDevice", __LINE__, 0, [&] { return hipSetDevice(device); });
    if (he == hipSuccess) he = take_stream(device, &e->own_stream);
    if (he == hipSuccess) he = sc_dev_malloc(e->state.out(), (size_t)e->npitch * 4);
    if (he != hipSuccess)
        return fail(he == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_DEVICE, "engine setup failed: %s", hipGetErrorString(he));
    e->stream = e->own_stream;
    return SC_OK;
}

// The engine owns the x-planes  i0, i0 + istride, ...  (`planes` of them) of the global grid.
int create(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t i0, int64_t istride,
           int64_t planes, const float *origin, float vs, int mode, float default_value, int device, bool deferred = false) {
    if (!out) return fail(SC_ERR_INVALID, "null out pointer");
    *out = nullptr;
    if (!origin) return fail(SC_ERR_INVALID, "null origin");
    if (nx <= 0 || ny <= 0 || nz <= 0) return fail(SC_ERR_INVALID, "shape must be positive");
    // int -> float of an index must be exact
    if (nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24))
        return fail(SC_ERR_INVALID, "axis longer than 2^24 voxels");
    if (i0 < 0 || istride < 1 || planes < 1 || i0 + (planes - 1) * istride >= nx)
        return fail(SC_ERR_INVALID, "bad slab / plane set (first %lld, stride %lld, planes %lld of %lld)",
                    (long long)i0, (long long)istride, (long long)planes, (long long)nx);
    if (mode != SC_MODE_CARVE && mode != SC_MODE_AVERAGE)
        return fail(SC_ERR_INVALID, "unknown mode %d", mode);
    sc_engine *e = new (std::nothrow) sc_engine();
    if (!e) return fail(SC_ERR_NOMEM, "host allocation failed");
    e->device = device;
    e->mode = mode;
    e->nx = nx; e->ny = ny; e->nz = nz; e->i0 = i0; e->istride = istride; e->planes = planes;
    e->n = planes * ny * nz;
    e->nzp = (nz + 63) / 64 * 64;
    e->npitch = planes * ny * e->nzp;
    memcpy(e->origin, origin, sizeof e->origin);
    e->vs = vs;
    e->default_value = default_value;
    e->fresh = true;
    if (deferred) {
        // the device half on a thread of its own: the caller goes on (reads its files, decodes them) and the first
        // call that needs the device joins -- and takes the failure, if there is one
        e->setup_pending = true;
        try {
            e->setup_thread = std::thread([e]() {
                e->setup_rc = device_setup(e);
                if (e->setup_rc != SC_OK) e->setup_err = g_err;  // (the thread's own message)
            });
        } catch (...) {
            e->setup_pending = false;
            int rc = device_setup(e);
            if (rc) {
                sc_destroy(e);
                return rc;
            }
        }
        *out = e;
        return SC_OK;
    }
    int rc = device_setup(e);
    if (rc) {
        sc_destroy(e);
        return rc;
    }
    *out = e;
    return SC_OK;
}

}  // namespace
