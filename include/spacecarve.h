/*
 * spacecarve.h -- C ABI of the MI355X (gfx950) voxel back-projection engine.
 *
 * This is the drop-in boundary for the reference's device layer: everything
 * plant3dvision/cl.py::Backprojection does with PyOpenCL (cl.py:118-311) maps onto
 * the entry points below, and nothing else of plant-3d-vision is replaced.  Plain
 * pointers and sizes only; no torch / HIP types in any signature.  The host-side
 * mirror (plant-3d-vision_amd/cl.py) binds these with cffi (ABI mode) or ctypes;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions (all from the reference):
 *   - grid state is C-order [nx][ny][nz], z fastest   (kernels/common.h:1-12)
 *   - carve state int32 in {-1 carved, 0 unseen, 1 kept} (kernels/backprojection.c:67-83)
 *   - average state float32 running sum in view order    (kernels/backprojection.c:54)
 *   - K = [fx, fy, cx, cy], R row-major 3x3, t: float32   (cl.py:293-296)
 *   - masks are row-major [H][W]; u = column, v = row     (cl.py:217)
 *   - arithmetic: IEEE binary32, no contraction, correctly rounded divide,
 *     (int) cast rejecting NaN/inf/out-of-range
 *
 * Threading: an engine is driven by one host thread at a time (calls on it may come from different
 * threads one after the other -- every entry selects the engine's device first); different engines
 * may be driven from different threads at once.  Every call
 * returns SC_OK (0) or a negative code; sc_last_error() gives the thread-local
 * message of the most recent failure.
 */
#ifndef SPACECARVE_H
#define SPACECARVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 1

/* error codes */
#define SC_OK 0
#define SC_ERR_INVALID (-1)   /* bad argument                        */
#define SC_ERR_DEVICE (-2)    /* HIP runtime error / no gfx950 device */
#define SC_ERR_NOMEM (-3)     /* host or device allocation failed     */
#define SC_ERR_STATE (-4)     /* call not valid in the engine's state */

/* sc_create mode -- replaces the kernel choice at cl.py:145-152 */
#define SC_MODE_CARVE 0   /* `carve`,   int32 state   (backprojection.c:57-84) */
#define SC_MODE_AVERAGE 1 /* `average`, float32 state (backprojection.c:36-55) */

/* mask element types accepted by sc_process_view* */
#define SC_MASK_U8 0  /* carve: foreground = (value != 0), the test at backprojection.c:79 */
#define SC_MASK_I32 1 /* carve: what cl.py:215 casts to                                    */
#define SC_MASK_F32 2 /* average: the value added at backprojection.c:54                   */
#define SC_MASK_U8_INV 3   /* carve: uint8 mask to be inverted first, i.e. `np.invert(mask)` of
                              cl.py:300-301 done on the device: foreground = (value != 255)   */
#define SC_MASK_BOOL_INV 4 /* carve: bool mask (bytes 0/1) to be inverted first (logical not):
                              foreground = (value == 0)                                       */
#define SC_MASK_U8_LUT 5   /* average: the ORIGINAL uint8 mask; the value added is table[byte],
                              the table (sc_set_lut) being what the host conversion of
                              cl.py:205-208 (img_as_float32, log) makes of each byte value      */

/* sc_set_option keys */
#define SC_OPT_VIEWS_PER_LAUNCH 1 /* 0 (default): defer views, fuse all pending views into one
                                     launch at flush; n>0: launch every n views (1 = one launch
                                     per view, the reference's schedule cl.py:223-226)        */
#define SC_OPT_VIEW_ORDER 2       /* carve only. 0: as given; 1 (default): inside a fused launch,
                                     most-perpendicular-first order (legal: the carve state is
                                     order-independent). average always keeps
                                     the given order (float sum).                             */
#define SC_OPT_TIME_KERNELS 3     /* 1: bracket every kernel launch with HIP events on the
                                     engine's stream; read with sc_kernel_stats.  2: only the
                                     carve / average kernel of a per-view launch and one pair
                                     around each fused batch, SC_KERNEL_STEP (an event pair costs
                                     a few microseconds of stream time)                       */
#define SC_OPT_MAX_PENDING 4      /* deferred views that force a flush (default 256)          */
#define SC_OPT_RESERVE_EVENTS 31  /* with SC_OPT_TIME_KERNELS: create n HIP events now (0..65536) so that the timed
                                     launches that follow find them in the engine's pool instead of creating them */
/* The fused carve's tuning knobs (SC_OPT_COMPACT .. SC_OPT_UNIT_CULL: where work moves between its kernels; results
 * never depend on them) are sc_set_option keys too, declared in spacecarve_tuning.h (included at the end of this
 * header) -- not part of what a caller of the reference's interface needs. */

/* kernel ids for sc_kernel_stats */
#define SC_KERNEL_CARVE 0
#define SC_KERNEL_AVERAGE 1
#define SC_KERNEL_PACK 2
#define SC_KERNEL_FILL 3
#define SC_KERNEL_LIST 4 /* confirm + special kernel + survivor-list stages of a fused carve */
#define SC_KERNEL_FLAGS 5 /* brick emptiness verdicts ahead of the dense stage (brick form) */
#define SC_KERNEL_STEP 6  /* a whole fused batch: mask packing + every kernel of its launch     */

typedef struct sc_engine sc_engine;

int sc_abi_version(void);
const char *sc_last_error(void);
/* number of visible HIP devices whose architecture is gfx950 (others are skipped); sc_create*
 * take a HIP ordinal and check that device alone */
int sc_device_count(int *count);

/*
 * Create an engine owning the whole grid.  Replaces Backprojection.__init__ +
 * init_buffers (cl.py:118-188): state = default_value everywhere (cl.py:173-175),
 * volinfo = {origin, voxel_size} as float32 (cl.py:181-183), shape (cl.py:185-187).
 * device: HIP device ordinal.
 */
int sc_create(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, const float origin[3],
              float voxel_size, int mode, float default_value, int device);

/*
 * Same, but the engine owns only the X-slab i in [i0, i1) of the global grid
 * (multi-GPU sharding).  Voxel coordinates are still computed from
 * the GLOBAL index (origin_x + (float)i * voxel_size), never from a shifted origin.
 * State / sc_get_values cover (i1-i0)*ny*nz elements.
 */
int sc_create_slab(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t i0, int64_t i1,
                   const float origin[3], float voxel_size, int mode, float default_value,
                   int device);

/*
 * Same, but the engine owns the x-planes  first, first + stride, first + 2*stride, ...  of the
 * global grid (plane-cyclic sharding: rank r of W takes first = r, stride = W).  An object in
 * the middle of the grid then loads every rank alike, which contiguous slabs do not.  State /
 * sc_get_values are [planes][ny][nz] in that order.
 */
int sc_create_cyclic(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t first, int64_t stride,
                     const float origin[3], float voxel_size, int mode, float default_value,
                     int device);

/*
 * The three above in one call, with flags: the engine owns `planes` x-planes first, first + stride, ... of the grid
 * (sc_create: 0, 1, nx; sc_create_slab: i0, 1, i1 - i0; sc_create_cyclic: first, stride, ceil((nx - first) / stride)).
 * SC_CREATE_DEFERRED (round 6): the arguments are judged now, the DEVICE half of the set-up -- runtime initialisation,
 * the process's first stream, the state's allocation: 130-240 ms in a fresh process, where cl.py:29-30 pays its context
 * and queue at import -- runs on a thread of the library's; the call returns at once, every later call that needs the
 * device joins that thread first and reports ITS failure (no device, not a gfx950, out of memory) as its own, and
 * sc_process_png_views decodes its files beside it: a cold `Voxels.run` (tasks/cl.py:100, 162-165) hides the decode
 * and whatever else the host does between the two calls behind the set-up.
 */
/* What cl.py:29-30 does at import (the context and the queue), without blocking the importer: a thread of the library's
 * initialises the runtime on `device` and creates its first stream; the first engine there takes that stream.  Returns
 * at once; a failure is the first engine's to report. */
int sc_prewarm(int device);
void sc_prewarm_wait(void); /* returns when no such thread is running any more: call it before the process exits */
#define SC_CREATE_DEFERRED 1
int sc_create_ex(sc_engine **out, int64_t nx, int64_t ny, int64_t nz, int64_t first, int64_t stride, int64_t planes,
                 const float origin[3], float voxel_size, int mode, float default_value, int device, int flags);

/* Diagnostic of a (deferred) engine's set-up: out[0] = milliseconds its device half took, out[1] = milliseconds the first
 * call that needed the device waited for it. */
int sc_setup_times(sc_engine *e, double out[2]);

void sc_destroy(sc_engine *e);

/* Backprojection.clear (cl.py:307-311): reset state to default_value, drop pending views. */
int sc_clear(sc_engine *e);

int sc_set_option(sc_engine *e, int key, int64_t value);

/* Averaging engines: the 256-entry float32 table used by SC_MASK_U8_LUT views enqueued
 * afterwards (views already enqueued are flushed with the previous table). */
int sc_set_lut(sc_engine *e, const float *lut256);

/* Run the engine's work on an existing hipStream_t (a non-default stream of the caller);
 * NULL restores the engine's own stream.  The engine's own stream is non-blocking: it does not
 * synchronise with the legacy default stream (handle 0, which is what torch's default stream
 * is), so a caller whose masks are produced there uses sc_order_after instead. */
int sc_set_stream(sc_engine *e, void *hip_stream);

/* Order everything the engine enqueues from now on AFTER the work enqueued so far on
 * `producer_stream` (a hipStream_t; NULL = the legacy default stream): an event recorded there
 * and waited for on the engine's stream.  For device-resident masks another stream is still
 * writing (sc_process_views_device); replaces nothing in the reference, whose single in-order
 * queue (cl.py:29-30) has no such hazard. */
int sc_order_after(sc_engine *e, void *producer_stream);

/* The other direction: everything enqueued from now on on `consumer_stream` (NULL = the legacy default stream)
 * runs AFTER the work the engine has enqueued so far -- for a consumer on another stream of what the engine
 * leaves in device memory (sc_values_device_ptr, sc_values_packed), and for a producer who wants to reuse a
 * buffer handed to sc_process_views_device, without waiting on the host. */
int sc_order_before(sc_engine *e, void *consumer_stream);

/*
 * Backprojection.process_view (cl.py:190-227): one view from a HOST mask.
 * The mask is consumed before the call returns (the caller may free it); the kernel
 * launch itself may be deferred (SC_OPT_VIEWS_PER_LAUNCH).  row_stride_bytes = 0 means
 * tightly packed rows.  mask_dtype must fit the mode (U8/I32 carve, F32 average).
 * Carve masks (cl.py:215 + backprojection.c:79: a pixel counts when it is != 0) are reduced to 1 bit per pixel on
 * the library's host threads during the call and cross PCIe as bits, one copy per flush (sc_hostpack_bits is that
 * bit form by itself; SC_OPT_HOST_PACK 0: the bytes travel and are packed on the device).
 * Picture sizes: 1 <= H <= 2^24 - 32, 1 <= W <= 2^24, H W <= 2^34; else SC_ERR_INVALID ("bad mask shape").
 * Averaging masks are re-laid in strips of 128-byte tiles on the device, whose addressing is narrower:
 * uint8 masks with a table (SC_MASK_U8_LUT: tiles of 16 x 8 pixels) need ceil(H / 8) * 128 < 2^24 (H < 1 048 576) and
 * ceil(W / 16) * ceil(H / 8) * 128 < 2^31 bytes per view; float32 masks (SC_MASK_F32: tiles of 8 x 4 pixels) need
 * ceil(H / 4) * 32 < 2^24 (H < 2 097 152) and ceil(W / 8) * ceil(H / 4) * 128 < 2^33 bytes per view; beyond that
 * SC_ERR_INVALID.  sc_process_png_views takes files of at most 2^24 x 2^24 pixels and H W <= 2^31.
 */
int sc_process_view(sc_engine *e, const float K[4], const float R[9], const float t[3],
                    const void *mask, int H, int W, int mask_dtype, int64_t row_stride_bytes);

/* The file loop of Backprojection.process_label in one call (cl.py:282-303, for a carve engine and masks stored as
 * 8-bit greyscale PNG -- what `io.write_image(f, im, 'png')` makes of tasks/proc2d.py's uint8 masks and what
 * plantdb.io.read_image decodes for cl.py:298): V ENCODED files (png[q], sizes[q] bytes) with their poses, decoded on
 * `threads` host threads of this call's own (<= 0: 16), each mask reduced to bits as it comes out of the decoder
 * (invert != 0: np.invert on the uint8 pixels first, cl.py:300-301), the views enqueued in the order given.
 * SC_ERR_INVALID, and nothing enqueued, if a file is not a PNG this decoder takes (sc_png_info) or is damaged. */
int sc_process_png_views(sc_engine *e, int V, const float *K, const float *R, const float *t, const void *const *png,
                         const int64_t *sizes, int invert, int threads);

/* V views at once: K[V*4], R[V*9], t[V*3], masks[V] host pointers, common H, W, dtype. */
int sc_process_views(sc_engine *e, int V, const float *K, const float *R, const float *t,
                     const void *const *masks, int H, int W, int mask_dtype,
                     int64_t row_stride_bytes);

/*
 * V views whose masks are already resident in device memory on the engine's device,
 * contiguous [V][H][W] (the Masks2D / bench path: no host round trip).  The masks are read on the
 * engine's stream when the batch is launched (a fused batch packs them at the flush, part of them beside its
 * dense stage), and sc_flush only enqueues: the buffer must stay valid AND UNCHANGED until sc_synchronize or
 * sc_get_values* returns -- or until the caller has ordered its own stream behind the engine's work.
 */
int sc_process_views_device(sc_engine *e, int V, const float *K, const float *R, const float *t,
                            const void *masks_dev, int H, int W, int mask_dtype);

/*
 * The labels of one scan at once: L averaging engines of one grid on one device (one per label, each with its
 * table, sc_set_lut), V views with ONE set of poses, masks_dev[l] = label l's uint8 masks [V][H][W] in device
 * memory (SC_MASK_U8_LUT).  The reference runs the view loop once per label over the same cameras
 * (Backprojection.process_fileset, cl.py:248-255); here a voxel is projected once per view and every label's
 * mask is read at that pixel -- each label's sum is the same additions in the same order as its own
 * sc_process_views_device + sc_flush would make, bit for bit.  Launches at once (asynchronous); every engine's
 * stream is ordered behind the work.  Engines or masks that do not fit the one-launch form (different grids or
 * freshness, views pending, rows that are not whole 16-byte groups) are processed label by label instead.
 */
int sc_average_labels(sc_engine *const *engines, int L, int V, const float *K, const float *R, const float *t,
                      const void *const *masks_dev, int H, int W);
/* How many sc_average_labels calls of this process took the shared-launch form (the others went label by label:
 * more than 4 labels left over, masks or widths that are not 16-byte multiples, engines that differ): tests assert
 * the form they mean to exercise. */
int64_t sc_average_labels_fused_count(void);

/* Launch everything still deferred (asynchronous on the engine's stream). */
int sc_flush(sc_engine *e);
/* sc_flush + wait for the stream: the role of queue.finish() (cl.py:226). */
int sc_synchronize(sc_engine *e);

/*
 * Backprojection.get_values (cl.py:229-232): flush, wait, copy the state to `out`
 * (int32 or float32, C-order, (i1-i0)*ny*nz elements).
 */
int sc_get_values(sc_engine *e, void *out);

/*
 * The same read-back for carve labels as int8 (labels are -1 / 0 / 1, or default_value where no view
 * reached; SC_ERR_STATE if default_value does not fit): a quarter of the bytes cross PCIe; the host
 * mirror widens them back to the int32 array cl.py:229-232 returns.  (i1-i0)*ny*nz bytes.
 */
int sc_get_values_i8(sc_engine *e, int8_t *out);

/* Flush and return a device pointer to the engine's values as planes * ny * nz contiguous elements; work may
 * still be running on the engine's stream.  When nz is a multiple of 64 this IS the state (valid until
 * sc_destroy, and it changes as views are applied, like the reference's buffer); otherwise the state's rows are
 * padded and the pointer is a SNAPSHOT without the padding, made on the engine's stream by this call: valid
 * until the next call that changes the state or takes another snapshot. */
int sc_values_device_ptr(sc_engine *e, void **ptr);

/*
 * Carve labels packed for the wire (multi-GPU assembly; no reference counterpart -- the reference
 * is single-device).  bits = 2: the three states, label & 3 (-1 -> 3, 0 -> 0, 1 -> 1; SC_ERR_STATE unless
 * default_value is one of them); bits = 1: the occupancy the consumer binarises to (label == 1, proc3d.py:515).
 * Voxel v of the engine's voxels (its planes in its own order, no padding) is at bit  bits * (v % (32 / bits))
 * of 32-bit word  v / (32 / bits).  sc_values_packed flushes, packs on the engine's stream into an engine-owned
 * device buffer (valid until the next sc_values_packed / sc_destroy; work may still be running) and returns it
 * with its size, sc_packed_bytes(voxels, bits): whole 16-byte groups.  sc_get_values_packed copies the words to
 * the host.  sc_unpack_labels is the other end of an all-gather of such buffers: `world` ranks' buffers
 * rank_bytes apart (rank r's planes are r, r + world, ... of the grid: partition 0; or the slab
 * [nx r / world, nx (r + 1) / world): partition 1) into ONE [nx][ny][nz] grid in global order on `device`,
 * as int8 (out_bytes 1) or int32 (4), on hip_stream (NULL: the legacy default stream).
 */
int64_t sc_packed_bytes(int64_t voxels, int bits);
int sc_values_packed(sc_engine *e, int bits, void **ptr, int64_t *bytes);
int sc_get_values_packed(sc_engine *e, int bits, void *out);
/* cl.py:229-232 get_values of a carve volume, the fast way round: the labels cross PCIe at 2 bits each, in pieces,
 * and the library's host pool (SC_OPT_HOST_THREADS; `threads` is ignored since round 4) widens the pieces that
 * have arrived into out[voxels] (int32, the array the reference returns) while the next ones are on their way --
 * 512 MiB of int32 in 3-4 ms on 8 threads.  The packed labels land in a page-locked buffer the engine keeps
 * (32 MiB at 512^3, allocated at the first call); `staging` / `staging_bytes` are ignored since round 4 and may be
 * NULL / 0 (round 3: a caller's pageable buffer -- a copy into pageable memory runs at a quarter of the rate).
 * SC_ERR_STATE unless default_value is one of -1, 0, 1 (use sc_get_values / sc_get_values_i8 then). */
int sc_get_values_wire2(sc_engine *e, int32_t *out, void *staging, int64_t staging_bytes, int threads);
/* Host code only (no device, no engine): the widening sc_get_values_wire2 does, by itself -- `voxels` labels at
 * 2 bits each in packed[(voxels + 15) / 16] (the layout above) into out[voxels] on the host pool (`threads` ignored). */
int sc_widen_labels2(const uint32_t *packed, int64_t voxels, int32_t *out, int threads);
/* Host code only: `world` ranks' packed planes (2 bits per label, rank-major, `rank_bytes` apart: what a gather of
 * the ranks' sc_values_packed buffers gives) into ONE int32 grid out[nx][ny][nz] in global plane order -- the host
 * end of ShardedBackprojection.gather_to_host (cl.py:229-232 get_values of a sharded run).  partition: 0 plane-cyclic
 * (plane i is plane i / world of rank i % world), 1 slabs.  On the library's host pool. */
int sc_widen_labels2_ranks(const uint32_t *packed, int64_t rank_bytes, int world, int partition, int64_t nx, int64_t ny,
                           int64_t nz, int32_t *out);
/* Host code only: the bit form in which sc_process_view sends a carve mask over PCIe (cl.py:215 + backprojection.c:79:
 * a pixel counts when it is != 0; SC_MASK_U8_INV / SC_MASK_BOOL_INV: after np.invert, cl.py:300-301) -- row-major,
 * out[H][(W + 31) / 32] words, pixel u of a row at bit u & 31 of word u >> 5, bits beyond W zero.  mask_dtype: the
 * carve dtypes (SC_MASK_U8, SC_MASK_I32, SC_MASK_U8_INV, SC_MASK_BOOL_INV); row_stride_bytes 0 = tight rows. */
int sc_hostpack_bits(const void *mask, int H, int W, int mask_dtype, int64_t row_stride_bytes, uint32_t *out);
int sc_unpack_labels(int device, void *hip_stream, const void *recv_dev, int64_t rank_bytes, int world, int partition,
                     int64_t nx, int64_t ny, int64_t nz, int bits, void *out_dev, int out_bytes);

/*
 * The BRICK-SPARSE transport form of carve labels (round 6; multi-GPU assembly; no reference counterpart:
 * the reference is single-device, cl.py:29-30 -- what the far end needs is what cl.py:229-232 returns, the labels).
 * A carved volume is uniform almost everywhere, and the engine already holds a 1-byte verdict per 16 x 64-voxel brick
 * of one x-plane (brick b = (plane * bricks_y + j / 16) * bricks_z + k / 64).  One rank's buffer:
 *     header   64 bytes: uint32 magic "SCSP", version 1, bits 2, nbricks, cap, nmixed, planes, ny, nz, bricks_y,
 *              bricks_z, first, stride (its planes are first, first + stride, ... of the grid), nread (bricks the sender had to read: diagnostic), 2 spare
 *     codes    [nbricks] bytes: 0 / 1 / 3 = every voxel of the brick is 0 / 1 / -1 (label & 3); 2 = MIXED   (to 64 bytes)
 *     ids      [cap] uint32: the brick of payload slot s                                       (cap is a multiple of 16)
 *     payload  [cap][256] bytes: slot s = the brick's labels at 2 bits each, voxel (column jl, depth kl) of the brick
 *              at bits 2 (v % 16) of word v / 16, v = jl * 64 + kl; voxels beyond ny / nz are 0
 * sc_sparse_bricks / sc_sparse_rank_bytes give the sizes (cap is clamped to [16, nbricks] and rounded up to 16).
 * sc_values_sparse flushes and packs on the engine's stream into an engine-owned device buffer (two alternate: the
 * buffer of a call stays untouched until the call after next) and returns it (work may still be running).  It reads
 * only bricks nothing settles: behind ONE fused batch on a cleared volume the batch's verdict bytes settle most
 * bricks and its live list names the others (one launch, a plant's 7 577 live bricks of 131 072: 31 MB read, 2 MB
 * written, where the dense 2-bit form writes 32 MiB); otherwise bricks an earlier launch found empty are skipped and
 * the rest is read.  A brick that is read and turns out uniform gets its code, not a slot.  cap = 0: the engine's
 * last capacity (first call: an eighth of the bricks).  nmixed > cap: slots were refused -- the codes are complete,
 * the payload is not; ask again with cap >= nmixed.  SC_ERR_STATE unless default_value is -1, 0 or 1.
 * sc_sparse_headers returns nmixed[r], cap[r] of the `world` buffers rank_bytes apart in device memory (every rank of
 * an all-gather sees the same numbers, so all ranks take the same decision about a retry without talking); it waits
 * for done_event -- the event sc_all_gather_sparse hands out, recorded behind ITS collective -- and copies on a stream
 * of the library's own, or (done_event NULL) copies on hip_stream behind whatever that stream still has to do.  sc_unpack_sparse writes ONE [nx][ny][nz] grid in global order from them on hip_stream:
 * out_kind 4 int32 labels, 1 int8 labels, 0 the uint8 occupancy label == 1 (what proc3d.py:515 binarises to).
 * sc_widen_sparse_ranks is the same on the host (no device) into int32, on the library's host pool.
 */
int64_t sc_sparse_bricks(int64_t planes, int64_t ny, int64_t nz);
int64_t sc_sparse_rank_bytes(int64_t nbricks, int64_t cap);
int sc_values_sparse(sc_engine *e, int64_t cap, void **ptr, int64_t *bytes);
int sc_get_values_sparse(sc_engine *e, int64_t cap, void *out, int64_t out_bytes);
int sc_sparse_headers(int device, void *hip_stream, void *done_event, const void *recv_dev, int64_t rank_bytes, int world,
                      uint32_t *nmixed, uint32_t *cap);
int sc_unpack_sparse(int device, void *hip_stream, const void *recv_dev, int64_t rank_bytes, int world, int64_t nx, int64_t ny,
                     int64_t nz, void *out_dev, int out_kind);
int sc_widen_sparse_ranks(const void *packed, int64_t rank_bytes, int world, int64_t nx, int64_t ny, int64_t nz, int32_t *out);

/*
 * RCCL behind the C ABI (round 6): one communicator per process and GPU, so that a carve rank assembles the grid without
 * torch.  librccl is opened at the first call (the copy already in the process, if any); rank 0 makes the 128-byte id
 * (sc_comm_unique_id) and hands it to the others by whatever means the host has (plant-3d-vision_amd/sharded.py: a TCP
 * socket on MASTER_ADDR / MASTER_PORT); sc_comm_create is collective (ncclCommInitRank).  The communicator owns a
 * non-blocking stream (sc_comm_stream) for collectives that run beside an engine's work.
 * sc_all_gather_sparse / sc_all_gather_packed: flush, pack the engine's labels (sc_values_sparse with the capacity EVERY
 * rank names alike / sc_values_packed) and all-gather `rank_stride` bytes per rank -- the size of the rank with the most
 * planes, the same on every rank -- into recv_dev[nranks][rank_stride].  overlap = 0: the collective is enqueued on the
 * engine's own stream.  overlap = 1: on the communicator's stream behind an event, and the engine's stream does not
 * wait -- the next batch's carve runs beside the collective; the engine waits by itself before it packs into a send
 * buffer a collective may still be reading.  The caller keeps recv_dev untouched until it has waited
 * (sc_comm_synchronize, sc_sparse_headers on the stream the collective ran on).
 */
typedef struct sc_comm sc_comm;
int sc_comm_available(void); /* SC_OK when librccl could be opened (nothing else is done) */
int sc_comm_unique_id(void *id, int64_t id_bytes /* >= 128 */);
int sc_comm_create(sc_comm **out, const void *id, int nranks, int rank, int device);
void sc_comm_destroy(sc_comm *c);
int sc_comm_size(const sc_comm *c);
int sc_comm_rank(const sc_comm *c);
int sc_comm_stream(sc_comm *c, void **hip_stream);
int sc_comm_synchronize(sc_comm *c);
int sc_comm_barrier(sc_comm *c); /* a 16-byte all-gather, waited for: every rank has called it when it returns */
int sc_comm_all_gather(sc_comm *c, const void *send_dev, void *recv_dev, int64_t bytes_per_rank, void *hip_stream /* NULL: its own */);
int sc_engine_stream(sc_engine *e, void **hip_stream);
int sc_all_gather_sparse(sc_engine *e, sc_comm *c, int64_t cap, void *recv_dev, int64_t rank_stride, int overlap,
                         void **done_event /* may be NULL; the engine's, valid until its next sc_all_gather_sparse but one */,
                         const void **headers_host /* may be NULL; likewise */);
/* The headers of THAT gather without a copy at the time of asking: sc_all_gather_sparse has put a copy of the ranks'
 * headers to page-locked host memory on the collective's stream, in front of done_event; this waits for the event
 * (host code: a poll) and reads them.  nmixed[r], cap[r] as sc_sparse_headers. */
int sc_sparse_wait_headers(void *done_event, const void *headers_host, int64_t rank_bytes, int world, uint32_t *nmixed,
                           uint32_t *cap);
int sc_all_gather_packed(sc_engine *e, sc_comm *c, int bits, void *recv_dev, int64_t rank_stride, int overlap);

/* number of voxels this engine owns */
int64_t sc_num_voxels(const sc_engine *e);

/* With SC_OPT_TIME_KERNELS: launches and summed HIP-event milliseconds per kernel id
 * since the last sc_reset_kernel_stats (waits for the stream). */
int sc_kernel_stats(sc_engine *e, int kernel_id, int64_t *launches, double *total_ms);
int sc_reset_kernel_stats(sc_engine *e);

/* One HIP event pair on the engine's stream around whatever the caller enqueues in between (any number
 * of batches): sc_span_begin records the first event where the stream stands, sc_span_end records the
 * second, waits for it and returns the milliseconds between them.  Unlike SC_OPT_TIME_KERNELS this puts
 * nothing between the batches (an event pair per batch is a barrier packet each, 3-5 us of stream time). */
int sc_span_begin(sc_engine *e);
int sc_span_end(sc_engine *e, double *ms);

/* Diagnostics of the last fused carve launch (waits for the stream): out[0] bricks no view found
 * empty (brick form, else 0), out[1] voxels alive after the dense stage, out[2] after the first
 * survivor stage, out[3] 1 if a survivor list overflowed (the special kernel's dense pass took over). */
int sc_fused_counts(sc_engine *e, int64_t out[4]);
/* ... the same four, then out[4]: candidate bricks (kept as they are by the views packed ahead) that a later
 * view did not keep -- carved unit by unit by the special kernel; out[5]: units on the bulk list
 * (SC_OPT_BULK_MIN); out[6]: their work items (0 when the batch had fewer units than SC_OPT_BULK_FLOOR: their
 * voxels took the ordinary lists); out[7]: 0 (round 3: batches the host kept the bulk list off). */
int sc_fused_counts_ex(sc_engine *e, int64_t out[8]);
/* What the last flushed batch packed of its masks, in 32x32 tiles (SC_OPT_PACK_REACH; all 0 for a batch that was not
 * packed at its flush): out[0] tiles packed ahead of the flags kernel, out[1] the tiles of those views' pictures,
 * out[2] tiles packed beside the dense stage (waits for the stream), out[3] the tiles of those views' pictures. */
int sc_pack_counts(sc_engine *e, int64_t out[4]);

/* Self-test: runs the kernels' shared-reciprocal division and the compiler's IEEE division on
 * `count` pseudo-random operand triples (mode 0: raw bit patterns, 1: projection-like
 * magnitudes) and reports how many quotients differ bit-for-bit (must be 0) and how many
 * triples took the fast path.  Mode 2: numerators of at most 2^-40 in magnitude (zero and denormals included) over
 * denominators and intrinsics of a certified view -- there the PIXEL and the picture test are compared, not the
 * quotient (csrc/sc_project.h says why that is what matters); every sample counts as fast. */
int sc_selftest_division(sc_engine *e, int64_t count, uint32_t seed, int mode,
                         uint64_t *mismatches, uint64_t *fast_pairs);

/*
 * Self-test of the projection the voxel kernels share (backproject_point, backprojection.c:3-34,
 * with the coordinates of :71-73): `count` samples, each a pose record and a voxel index, give
 * one result word each:  v * W + u + 1  when the reference would touch mask[v][u], 0 when it
 * rejects the point.  `poses`: nposes records of 28 32-bit words
 *   float K[4], R[9], t[3], origin[3], voxel_size;  int32 W, H, nx, ny, nz, 0, 0, 0.
 * Explicit samples: ijk[count][3] voxel indices (+ pose_idx[count], else record 0).
 * Hashed samples (ijk == NULL): record and voxel are drawn from (seed, sample index) by an
 * integer hash the caller can reproduce (oracle/spacecarve_oracle.c restates it), the record per
 * 64 consecutive samples, the voxel inside that record's nx x ny x nz grid.
 * words_out[count] and/or digests_out[ceil(count / 65536)] (sum over a run of 65536 samples of
 * mix32(word ^ (uint32)index)) receive the results.  The caller compares them with the reference
 * arithmetic; no reference counterpart (the reference has no tests on this function).
 */
int sc_selftest_project(sc_engine *e, int64_t count, uint32_t seed, int nposes, const float *poses,
                        const int32_t *ijk, const int32_t *pose_idx, uint32_t *words_out,
                        uint64_t *digests_out);

/*
 * Diagnostic (host code only, no device call): would a view with this pose take the kernels' certified
 * path on a grid of nx x ny x nz voxels with this origin and voxel size?  The host checks, in double precision and with wide margins, that every voxel centre of the grid
 * projects with 2^-10 < p_z and |p_x|, |p_y|, p_z < 2^30 and that the intrinsics are finite and below
 * 2^30; for such a view the projection (backprojection.c:11-31) spends two comparisons on the range test
 * of its shared-reciprocal division and two on the picture test instead of nine.  Results are the same
 * either way (tests/test_project_selftest.py runs both); *certified = 1 or 0.  No reference counterpart.
 */
int sc_view_certified(const float origin[3], float voxel_size, int64_t nx, int64_t ny, int64_t nz, const float K[4],
                      const float R[9], const float t[3], int *certified);

/*
 * The carve's immediate consumer: plant3dvision/proc3d.py::vol2pcd (:490-570, called by
 * tasks/proc3d.py:134) on the GPU.  volume: host pointer, or device pointer on `device` when
 * on_device != 0 (e.g. sc_values_device_ptr: the volume then never crosses PCIe); dtype 0 int32,
 * 1 float32, 2 float64, 3 uint8; C-order [nx][ny][nz].  gauss_w: the 5 distinct weights of
 * scipy's radius-4 Gaussian kernel (centre first), computed by the host as scipy does.
 * Returns malloc'ed float64 arrays [count][3] (release with sc_free_host): points in world
 * coordinates and unit normals, in C-order of the shell voxels; voxels whose gradient is zero
 * carry NaNs (the reference drops them afterwards, proc3d.py:559-561).
 */
int sc_vol2pcd(const void *volume, int on_device, int dtype, int64_t nx, int64_t ny, int64_t nz,
               const double origin[3], double voxel_size, double level_set_value,
               const double gauss_w[5], int device, double **points_out, double **normals_out,
               int64_t *count);
/* The same from carve labels in their PACKED, rank-major form -- what an all-gather of the ranks' sc_values_packed
 * buffers leaves on a device (`world` ranks x `rank_bytes`, `bits` 2 or 1 per label, `partition` 0 plane-cyclic /
 * 1 slabs: the arguments of sc_unpack_labels).  Labels are -1 / 0 / 1, so the reference's `volume > 0.5`
 * (proc3d.py:515) is `label == 1` and is read off the packed words: the full-size grid (1 GiB of int8 at 1024^3)
 * is never written.  Runs on the device's default stream: the caller has waited for the collective. */
int sc_vol2pcd_packed(const void *recv_dev, int64_t rank_bytes, int world, int partition, int bits, int64_t nx,
                      int64_t ny, int64_t nz, const double origin[3], double voxel_size, double level_set_value,
                      const double gauss_w[5], int device, double **points_out, double **normals_out, int64_t *count);
/* The same for ONE CLASS of a winner volume (sc_select_classes below): winner is uint8 [nx][ny][nz], on the host or on
 * `device` (on_device != 0, read in place on the device's default stream: the caller has waited for what wrote it);
 * the occupancy is `winner == cls` (cls 0..255), written by one kernel in front of the unchanged pipeline.  The result
 * is bit for bit that of sc_vol2pcd on the uint8 volume (winner == cls); slabs as for uint8 (1 byte per voxel). */
int sc_vol2pcd_class(const uint8_t *winner, int on_device, int cls, int64_t nx, int64_t ny, int64_t nz, const double origin[3],
                     double voxel_size, double level_set_value, const double gauss_w[5], int device, double **points_out,
                     double **normals_out, int64_t *count);
const char *sc_vol2pcd_last_error(void);
/* sc_vol2pcd keeps its device work buffers (49 bytes per voxel, per device) between calls while they are at most
 * 1 GiB (larger ones are freed when the call ends); this gives back what is kept.  The caller's current HIP
 * device is left as it was. */
void sc_vol2pcd_release(void);
/* Largest device work buffers a sc_vol2pcd call may take, in bytes (default 8 GiB; 0 = no limit).  A volume that
 * needs more (49 bytes per voxel) goes through in x-slabs with a halo of the pipeline's reach on either side:
 * same points, same order. */
void sc_vol2pcd_set_scratch_limit(int64_t bytes);
void sc_free_host(void *p);

/*
 * SegmentedPointCloud's scoring loop (plant3dvision/tasks/proc3d.py:203-232 over
 * proc3d.py::backproject_points :655-659) on the GPU: P float64 points, V views (K[V][4] =
 * fx,fy,cx,cy, R[V][9], t[V][3], float64), L label images per view, masks uint8 [L][V][H][W]
 * (host, or device when masks_on_device != 0).  Writes scores_out [L][P] (float64 sums of mask
 * values at int(pixel + 0.5)) and labels_out [P] = arg-max over labels (first maximum).
 */
int sc_label_points(const double *points, int64_t P, int L, int V, const double *K, const double *R,
                    const double *t, const void *masks, int masks_on_device, int H, int W, int device,
                    double *scores_out, int32_t *labels_out);
const char *sc_label_points_last_error(void);

/*
 * The geometric pipeline's mask producer: plant3dvision/tasks/proc2d.py::Masks.f (:224-249) over
 * plant3dvision/proc2d.py (:69-220) on the GPU.  rgb: uint8 [V][H][W][3] (R, G, B); per picture, independently:
 * imin / imax over all its bytes, x' = (x - imin) / (imax - imin) (min(x, 1) for a constant picture), then
 * linear  f = (c0 r' + c1 g') + c2 b'  or excess_green  s = ((r' + g') + b') + 1e-9, f = ((2 (g'/s)) - (r'/s)) - (b'/s),
 * all in IEEE binary64 without contraction; mask = f > threshold; `nsteps` (0..32) 3x3 dilation steps, one after the
 * other, out[p] = OR over the footprint's offsets o of in[p - o], outside the picture is background (the expanded
 * series of masks2d.disk_series(n)); masks_out: uint8 [V][H][W] of 0 / 255.  coefs are read for both filters and
 * used by the linear one.  Restates skimage's rescale_intensity from its source: parity unpinned.
 *
 * Device pointers on both sides (rgb_on_device, out_on_device != 0): the work is enqueued on hip_stream (NULL = the
 * legacy default stream) and the call returns without waiting, so sc_order_after(engine, hip_stream) +
 * sc_process_views_device(..., SC_MASK_U8) consumes the masks without a host wait.  A host pointer on either side
 * is staged by the library and the call returns when masks_out is complete.  ranges_out (host, [V][2] = imin, imax;
 * may be NULL) is a diagnostic and makes the call wait.
 * The work buffers (1 bit per pixel, 2 KiB per picture) are the library's, one set per device, kept between calls
 * and given back by sc_masks_release.  Every call is ordered on the device behind the previous call of that device
 * with an event, whatever the two streams: a call never writes into buffers an earlier one may still be reading.
 * Arguments are judged before any device call: V, H, W >= 1, 3 H W < 2^31, 0 <= nsteps <= 32, step ids 0..5,
 * filter 0..1, finite coefficients and threshold, non-NULL rgb / coefs / masks_out.
 */
#define SC_FILTER_LINEAR 0
#define SC_FILTER_EXCESS_GREEN 1
/* one 3x3 dilation step each, the footprints of masks2d._FOOTPRINTS */
#define SC_FOOT_T0 0
#define SC_FOOT_T90 1
#define SC_FOOT_T180 2
#define SC_FOOT_T270 3
#define SC_FOOT_DIAMOND 4
#define SC_FOOT_SQUARE 5
int sc_masks_from_rgb(const void *rgb, int rgb_on_device, int V, int H, int W, int filter, const double coefs[3],
                      double threshold, const uint8_t *steps, int nsteps, int device, void *hip_stream,
                      void *masks_out, int out_on_device, int32_t *ranges_out /* [V][2] imin, imax; may be NULL */);
const char *sc_masks_last_error(void);
/* Gives back the work buffers sc_masks_from_rgb keeps (after waiting for the work that uses them).  The caller's
 * current HIP device is left as it was. */
void sc_masks_release(void);

/*
 * The lens correction in front of the mask producer: plant3dvision/tasks/proc2d.py::Undistorted.f (:120-143) over
 * plant3dvision/proc2d.py::undistort (:25-66) = cv2.undistort(img, A, dist, None) on the GPU, for V pictures of ONE
 * camera.  rgb, rgb_out: uint8 [V][H][W][3]; K = fx, fy, cx, cy and dist = k1, k2, p1, p2, k3 as binary64 (a caller that
 * follows the reference rounds them through float32 first: plant3dvision/camera.py:104-128 makes float32 arrays).
 * Per output pixel (row i, column j), every operation IEEE binary64 in the order written, no contraction:
 *   x = (j - cx) / fx, y = (i - cy) / fy, x2 = x x, y2 = y y, r2 = x2 + y2, _2xy = (2 x) y,
 *   kr = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = (x kr + p1 _2xy) + p2 (r2 + 2 x2), yd = (y kr + p1 (r2 + 2 y2)) + p2 _2xy,
 *   u = fx xd + cx, v = fy yd + cy, iu = rint(32 u), iv = rint(32 v) (half to even).
 * A pixel with u or v not finite or |iu|, |iv| >= 2^30 is unmapped: output (0, 0, 0), map entry (INT32_MIN, INT32_MIN).
 * Otherwise sx = iu >> 5, sy = iv >> 5, a = iu & 31, b = iv & 31 and per channel, a tap outside the picture counting 0
 * (and never read),  out = ((32-a)(32-b) p(sy,sx) + a(32-b) p(sy,sx+1) + (32-a)b p(sy+1,sx) + ab p(sy+1,sx+1) + 512) >> 10.
 * Restates OpenCV's initUndistortRectifyMap (CV_16SC2, INTER_BITS 5) + remap(INTER_LINEAR, BORDER_CONSTANT 0) from its
 * published algorithm: parity unpinned, with two deviations (the ray is evaluated directly per pixel, not by running
 * sums along a row; sx, sy beyond +-32768 lie outside, no (short) wrap) -- DESIGN.md 17.
 *
 * Device pointers on both sides: the work is enqueued on hip_stream (NULL = the legacy default stream) and the call
 * returns without waiting, so sc_masks_from_rgb on the same stream consumes rgb_out without a host wait.  A host
 * pointer on either side is staged by the library and the call returns when rgb_out is complete.  map_out (host,
 * [H][W][2] = iu, iv; may be NULL) is a diagnostic and makes the call wait.  The work buffer (the map, 8 bytes per
 * pixel) is the library's, one per device, kept between calls, ordered across streams as sc_masks_from_rgb's are, given
 * back by sc_undistort_release (the caller's current HIP device is left as it was).
 * Judged before any device call (SC_ERR_INVALID): V, H, W >= 1, 3 H W < 2^31, non-NULL rgb / K / dist / rgb_out, all
 * nine numbers finite, fx and fy non-zero, rgb and rgb_out must not overlap.
 */
int sc_undistort_rgb(const void *rgb, int rgb_on_device, int V, int H, int W, const double K[4] /* fx fy cx cy */,
                     const double dist[5] /* k1 k2 p1 p2 k3 */, int device, void *hip_stream, void *rgb_out, int out_on_device,
                     int32_t *map_out /* [H][W][2] iu, iv; may be NULL */);
const char *sc_undistort_last_error(void);
void sc_undistort_release(void);

/*
 * The clustering of OrganSegmentation (plant3dvision/tasks/proc3d.py:419-521): what open3d's
 * cluster_dbscan(eps, min_points) computes for one cloud, on the GPU.  points: float64 [P][3]; labels_out: int32 [P],
 * cluster ids from 0, noise -1; nclusters_out (host, may be NULL): the number of clusters.  The rules, order-free:
 *   d2(i, j) = ((dx dx) + (dy dy)) + (dz dz) in IEEE binary64 without contraction; j is a neighbour of i iff
 *   d2(i, j) < eps * eps (strict, the product rounded once, i its own neighbour); i is core iff it has at least
 *   min_points neighbours (0 behaves as 1); clusters are the connected components of the core points, numbered by the
 *   rank of their smallest point index; a non-core point with core neighbours takes the smallest id among them;
 *   every other point is noise.
 * Restates open3d's sequential loop, which cannot be run here: parity unpinned.
 *
 * points_on_device / labels_on_device != 0: device pointers on `device`, read and written on hip_stream (NULL = the
 * legacy default stream).  The call waits once for its first kernel (which looks for non-finite coordinates) and,
 * when nclusters_out or a host pointer is given, for its last; with device pointers and nclusters_out == NULL it
 * returns with the remaining work enqueued.  The work buffers (about 100 bytes per point) are the library's, one set
 * per device, kept between calls, ordered across streams as sc_masks_from_rgb's are, given back by sc_dbscan_release.
 * Judged before any device call (SC_ERR_INVALID): NULL points / labels_out, P < 0 or P >= 2^31, eps not finite or
 * <= 0 (or eps * eps not a normal number), min_points < 0, a non-finite coordinate in host points -- a documented
 * deviation from open3d, which goes on computing.  In device points the first kernel finds it: SC_ERR_INVALID as
 * well, labels_out untouched.  P == 0 is SC_OK with 0 clusters and no device call.
 */
int sc_dbscan(const double *points, int points_on_device, int64_t P, double eps, int64_t min_points, int device,
              int32_t *labels_out, int labels_on_device, int32_t *nclusters_out, void *hip_stream);
const char *sc_dbscan_last_error(void);
/* Gives back the work buffers sc_dbscan keeps (after waiting for the work that uses them).  The caller's current
 * HIP device is left as it was. */
void sc_dbscan_release(void);

/*
 * The two evaluation tasks' counting passes on the GPU.
 *
 * sc_eval_voxels: what plant3dvision/tasks/evaluation.py::VoxelsEvaluation.evaluate (:421-477) counts.  pred and gt
 * are host arrays of L pointers to volumes in C order: the predictions all of shape (nx, ny, nz) and of pred_dtype
 * (SC_EVAL_F32 / SC_EVAL_F64), the ground truths all of shape (gx, gy, gz), every axis >= the prediction's, and of
 * gt_dtype (SC_EVAL_F32 / SC_EVAL_F64 / SC_EVAL_U8); only the corner [0:nx, 0:ny, 0:nz] of a ground truth is read.
 * The volumes are all in host memory (on_device == 0) or all device pointers on `device`, read in place on
 * hip_stream (NULL = the legacy default stream).  Per voxel, in IEEE binary64 (float32 is widened first):
 *   m = the first index of the greatest of the L predictions, v1 = that value, v2 = the greatest of the other L - 1;
 *   the voxel predicts class m iff v1 > min_contrast * v2 and none of its L values is NaN, and no other class.
 * For every class c other than `background` (an index, or -1 for none), with g = gt_c at the voxel: g > 0.5 counts
 * into tp (predicted) or fn, g < 0.5 into fp (predicted) or tn; g == 0.5 or NaN counts nowhere.  The reference
 * hard-codes min_contrast = 10.
 * counts_out (host): int64 [L][4] = tp, fp, tn, fn; the background's row is zero; gt[background] is not read and
 * may be NULL.  projection_out (host, may be NULL): uint8 [L][ny][nz], 1 where some x of the column predicts the
 * class (prediction_c.max(0), :455); the background's plane is zero.  The call returns when both are complete.
 * Counts are integers: two calls agree exactly.
 * Host volumes go through in x-slabs of whole planes (for a ground truth whole gy x gz planes) copied into the
 * unit's work buffer, whose size sc_eval_set_chunk_bytes bounds (default 256 MiB; <= 0 restores the default; one
 * x-plane of all volumes is taken as one slab even where it is larger).  A slabbed call counts what one piece counts.
 * Judged before any device call (SC_ERR_INVALID): NULL pointers, L outside 2..32 (the reference fails at L = 1),
 * dtype codes, background outside -1..L-1, an axis < 1 or >= 2^31, a ground truth smaller than the prediction.
 *
 * sc_eval_masks: plant3dvision/metrics.py::MaskEvaluator.evaluate (:246-272) for a stack of pictures.  gt and pred:
 * uint8 [n][H][W], both on the host or both on `device` (read in place on hip_stream).  Per picture: p = pred != 0
 * dilated dilation_amount times by the 4-connected cross with background outside the picture (binary_dilation's
 * default structure and border_value; any amount >= 0), g = gt != 0; counts_out (host): int64 [n][4] in the
 * reference's order tp, fn, tn, fp.  The call returns when counts_out is complete.  Host pictures go through in
 * batches of whole pictures within the same bound.  Judged before any device call: NULL pointers, n, H or W < 1,
 * H W >= 2^31, a negative dilation_amount.
 *
 * The work buffers are the library's, one set per device, kept between calls, ordered across streams as
 * sc_masks_from_rgb's are, given back by sc_eval_release (the caller's current HIP device is left as it was).
 */
#define SC_EVAL_F32 1
#define SC_EVAL_F64 2
#define SC_EVAL_U8 3
int sc_eval_voxels(const void *const *pred, int pred_dtype, const void *const *gt, int gt_dtype, int L, int64_t nx, int64_t ny,
                   int64_t nz, int64_t gx, int64_t gy, int64_t gz, int background, double min_contrast, int on_device, int device,
                   void *hip_stream, int64_t *counts_out, uint8_t *projection_out);
int sc_eval_masks(const void *gt, const void *pred, int on_device, int n, int H, int W, int dilation_amount, int device,
                  void *hip_stream, int64_t *counts_out);
void sc_eval_set_chunk_bytes(int64_t bytes);
const char *sc_eval_last_error(void);
void sc_eval_release(void);

/*
 * The decision step of the multiclass PointCloud task (plant3dvision/tasks/proc3d.py::PointCloud.run :84-115) on the
 * GPU: L class volumes -> ONE winner volume.  volumes: a host array of L pointers to volumes in C
 * order, all of shape (nx, ny, nz) and of `dtype` (SC_EVAL_F32 / SC_EVAL_F64 / SC_EVAL_U8), in the order of the
 * reference's `l = list(voxels.keys())`; `background` is the index of the key 'background', or -1 without one.
 * The rule, per voxel, every value taken to IEEE binary64 and the background's value multiplied by background_prior
 * in binary64 first (:89):
 *   m  = np.argmax over the L values (:93): the first index of the greatest value; if any value is NaN, the index of
 *        the first NaN;
 *   v2 = np.max of the other L - 1 values (:110): NaN if any of them is NaN;
 *   the voxel belongs to class m iff all three hold:
 *     m != background;
 *     min_contrast > 1.0 is false, or 1.0 > min_contrast * v2 (product and comparison in binary64; a NaN product
 *       compares false) (:113-114, where pred_c is the boolean res_idx == i, so `pred_c > x` is `1 > x` where it is
 *       true and irrelevant where it is false);
 *     1.0 > min_score (:115);
 *   it belongs to no other class, and to none if a test fails.
 * winner: uint8 [nx][ny][nz], the class index m or 255 for "no class": the reference's volume of class c is
 * `winner == c`.  counts (host, int64 [L]): the voxels of each class, 0 for the background.
 * volumes and winner are both in host memory (on_device == 0) or both device pointers on `device`, read and written
 * in place on hip_stream (NULL = the legacy default stream).  The call returns when the counts (and a host winner) are
 * complete.  Host volumes go through in x-slabs of whole planes copied into the unit's work buffer, whose size
 * sc_select_set_chunk_bytes bounds (default 256 MiB; <= 0 restores the default; one x-plane of all volumes is taken
 * as one slab even where it is larger); a slabbed call writes what one piece writes.
 * Judged before any device call (SC_ERR_INVALID): NULL pointers, L outside 2..32 (with one key the reference takes
 * its single-volume branch), the dtype code, background outside -1..L-1, an axis < 1 or >= 2^31.
 * The work buffers are the library's, one set per device, kept between calls, ordered across streams as
 * sc_masks_from_rgb's are, given back by sc_select_release.  Both leave the caller's current HIP device as it was.
 */
int sc_select_classes(const void *const *volumes, int dtype, int L, int background /* index, -1: none */, int64_t nx, int64_t ny,
                      int64_t nz, double background_prior, double min_contrast, double min_score, int on_device, int device,
                      void *hip_stream, uint8_t *winner, int64_t *counts /* host, L */);
void sc_select_set_chunk_bytes(int64_t bytes);
const char *sc_select_last_error(void);
void sc_select_release(void);

/*
 * The nearest point of another cloud, for the point-cloud evaluations: what open3d's
 * compute_point_cloud_distance, evaluate_registration and the KDTreeFlann loop of CompareSegmentedPointClouds compute
 * (plant3dvision/metrics.py:16-95, :384-519; tasks/evaluation.py:278-353), on the GPU.  queries: float64 [Q][3],
 * targets: float64 [P][3].  The rules, order-free (nanoflann's search cannot be run here: parity unpinned):
 *   N1. d2(q, t) = ((dx dx) + (dy dy)) + (dz dz) in IEEE binary64 without contraction, dx = qx - tx;
 *   N2. the nearest target of q is the t of least d2; among equal d2 the smallest target index wins;
 *   N3. with max_distance > 0 a query is matched iff d2 < max_distance * max_distance (strict, the product rounded
 *       once); an unmatched query reports index -1 and d2 = +inf; without it every query is matched when P > 0;
 *   N4. P == 0: every index -1 and every d2 +inf; Q == 0: nothing written; neither makes a device call (P == 0 with
 *       device outputs is therefore refused);
 *   N5. deviations: non-finite coordinates are refused (in host arrays before any device call, naming the first bad
 *       point; in device arrays by the first kernels), and so is a max_distance that is NaN or infinite or whose
 *       square is not a normal number;
 *   N6. sums_out = {n, sum d2, sum sqrt(d2)} over the matched queries, added in an order that depends on Q alone (a
 *       tree per block, the block partials by a tree): two calls give the same bits; no floating-point atomics.
 * The search is exact for every finite input: a dense grid over the targets' bounding box (at most 2^22 cells), rings
 * of cells around the query's cell until a proved lower bound on what is unvisited exceeds the best d2 strictly, and
 * for queries that four rings do not settle a pass over all P targets, one wavefront per query: O(P) per query at most.
 *
 * index_out [Q] int32 and d2_out [Q] double may each be NULL; both live where out_on_device says.
 * sums_out: NULL, or 3 host doubles {n matched, sum d2, sum sqrt(d2)}: the call then ends in a wait.
 * max_distance <= 0 means unbounded (N3).  queries_on_device / targets_on_device != 0: device pointers on `device`,
 * read in place on hip_stream (NULL = the legacy default stream).  The call waits once mid-way (the finite flags and
 * the targets' box) and, with sums_out or host outputs, at its end; otherwise it returns with the rest enqueued.
 * Judged before any device call (SC_ERR_INVALID): NULL queries / targets (with Q / P > 0), all three outputs NULL, Q or
 * P outside 0 .. 2^31 - 1, max_distance as in N5, the device ordinal, non-finite coordinates in host arrays.
 *
 * sc_nearest_confusion: counts_out: L*L host int64, counts[a*L + b] = queries with label a whose nearest target has
 * label b; queries with index -1 are not counted.  index and query_labels ([Q] int32) live where on_device says,
 * target_labels ([P] int32) where target_labels_on_device says.  Labels outside 0..L-1 -- and an index outside
 * -1..P-1 -- are refused (a flag kernel for device arrays; counts_out is zero then).  1 <= L <= 4096; tables with
 * L*L <= 1024 are gathered per block in LDS, larger ones by 64-bit integer atomics in global memory: the counts are
 * exact either way.  The call returns when counts_out is complete.
 *
 * The work buffers (28 bytes per target, 4 per query, three cell tables of at most 16 MiB, staging for host arrays) are the library's, one
 * set per device, shared by both entries, kept between calls, ordered across streams as sc_masks_from_rgb's are, given
 * back by sc_nearest_release (the caller's current HIP device is left as it was).
 */
int sc_nearest(const double *queries, int queries_on_device, int64_t Q,
               const double *targets, int targets_on_device, int64_t P,
               double max_distance, int device,
               int32_t *index_out, double *d2_out, int out_on_device,
               double *sums_out, void *hip_stream);
int sc_nearest_confusion(const int32_t *index, const int32_t *query_labels, int on_device, int64_t Q,
                         const int32_t *target_labels, int target_labels_on_device, int64_t P,
                         int L, int device, int64_t *counts_out, void *hip_stream);
const char *sc_nearest_last_error(void);
void sc_nearest_release(void);

/*
 * The k nearest points of another cloud: what open3d's KDTreeFlann.search_knn_vector_3d(p, k) computes
 * for the reference's knn_graph (plant3dvision/proc3d.py:160-183) and the stem walk of
 * angles_and_internodes_from_point_cloud (plant3dvision/arabidopsis.py:417-433), for Q queries at once, on the GPU.
 * Parity unpinned as above: the rules restate nanoflann's search in an order-free form.
 *   K1. d2 is N1's, bit for bit;
 *   K2. the key of a target is (d2, index), compared lexicographically; the answer for a query is the
 *       min(k, matched targets) smallest keys IN RISING KEY ORDER.  Keys are distinct, so the answer does not depend
 *       on the order of visiting; a tie at the k-th place goes to the smaller index;
 *   K3. with max_distance > 0 only targets with d2 < max_distance * max_distance count (strict, the product rounded
 *       once, as N3);
 *   K4. row q of index_out and d2_out has k places; the unused ones, after the used ones, hold index -1 and
 *       d2 = +inf.  P == 0: every place is unused and no device call is made (device outputs are refused then);
 *       Q == 0: nothing is written;
 *   K5. refused (SC_ERR_INVALID, before any device call): what N5 and sc_nearest refuse, k outside 1 .. SC_KNN_MAX,
 *       Q * k >= 2^31, a NULL index_out or d2_out.  Non-finite coordinates in device arrays are refused by the first
 *       kernels, as in sc_nearest;
 *   K6. k == 1 gives exactly sc_nearest's index and d2.
 * The search is exact for every finite input: sc_nearest's grid, planned for about `aim` targets per cell (a function
 * of k), one wavefront per query with its sorted list of k keys in LDS (12 k bytes), rings of cells until the proved
 * lower bound on what is unvisited exceeds the k-th d2 strictly, and for queries that four rings do not settle a pass
 * over all P targets, one wavefront per query.
 *
 * index_out [Q][k] int32 and d2_out [Q][k] double live where out_on_device says.  far_out: NULL, or one host int64
 * that receives the number of queries the pass over all targets took: the call then ends in a wait, as it does with
 * host outputs; otherwise it returns with the rest enqueued after its one mid-way wait (the finite flags and the box).
 * Errors are read with sc_nearest_last_error; the work buffers are sc_nearest's (plus 12 k bytes per query for host
 * outputs) and sc_nearest_release gives them back.
 * sc_knn_set_aim: the targets per cell the grid aims at, for measurements (tools/bench_knn.py); 0 restores the
 * built-in function of k.  No answer depends on it.
 */
#define SC_KNN_MAX 512 /* the reference's largest k (300) rounded up to a power of two */
int sc_knn(const double *queries, int queries_on_device, int64_t Q,
           const double *targets, int targets_on_device, int64_t P,
           int k, double max_distance, int device,
           int32_t *index_out /* [Q, k] */, double *d2_out /* [Q, k] */, int out_on_device,
           int64_t *far_out /* host, may be null */, void *hip_stream);
void sc_knn_set_aim(int aim);

/*
 * All points of another cloud within a radius: what open3d's KDTreeFlann.search_radius_vector_3d(p, r)
 * computes for the reference's radius_graph (plant3dvision/proc3d.py:186-209), for Q queries at once, on the GPU.
 * Parity unpinned as above: nanoflann's RadiusResultSet restated in an order-free form.
 *   R1. d2 is N1's, bit for bit;
 *   R2. target t is a neighbour of query q iff d2(q, t) < fl(radius * radius): strict, the product rounded once (a
 *       target at exactly `radius` is not a neighbour); this is N3 and sc_dbscan's rule 2;
 *   R3. row q holds ALL its neighbours in rising key (d2, index), compared lexicographically; keys are distinct, so
 *       the row does not depend on the order of visiting;
 *   R4. the answer is in CSR form: offsets int64 [Q + 1], offsets[0] = 0, offsets[q + 1] - offsets[q] the length of
 *       row q; index int32 [E] and d2 double [E], E = offsets[Q]; counts int32 [Q], the lengths alone.  Q == 0:
 *       offsets = {0}; P == 0: every count 0; neither makes a device call (device outputs are refused then);
 *   R5. refused (SC_ERR_INVALID, before the first device call wherever a host can judge): non-finite coordinates (host
 *       arrays naming the first bad point, device arrays by the first kernels as in sc_nearest), a radius that is not
 *       finite and positive (there is no "unbounded" here) or whose square is not a normal number, Q or P outside
 *       0 .. 2^31 - 1, NULL queries / targets / total_out, index_out without d2_out or the reverse, a negative
 *       capacity, the device ordinal;
 *   R6. capacity is the number of places in index_out and d2_out.  The call always computes the counts, the offsets and
 *       *total_out = E; it writes the rows iff capacity >= E.  With capacity < E it returns SC_OK, leaves index_out
 *       and d2_out untouched and still reports E: the caller asks once without rows, allocates, and asks again;
 *   R7. on one cloud searched against itself counts[i] >= min_points is exactly sc_dbscan's core test.
 * The search is exact for every finite input: sc_nearest's grid with an edge of at least the radius (so that rings 0
 * and 1 hold every neighbour in the ordinary case), one wavefront per query, rings of cells until the proved lower
 * bound on what is unvisited reaches radius^2 or nothing is unvisited -- no cap on the rings, no pass over all targets.
 * One launch counts, a scan makes the offsets, the call waits for E and the longest row, one launch fills: rows of up
 * to SC_RADIUS_LDS_ROW keys are sorted in LDS and written once, longer ones in place in global memory by a third
 * launch; *long_out (NULL, or one host int64: the call then ends in a wait) receives how many rows went that way.
 *
 * counts_out, offsets_out, index_out, d2_out may be NULL (the last two both or neither) and live where out_on_device
 * says.  The call waits twice (the finite flags and the box; E) and, with rows on the host or long_out, at its end.
 * Errors are read with sc_nearest_last_error; the work buffers are sc_knn's plus 4 Q bytes of counts, 8 (Q + 1) of
 * offsets and, for host rows, 12 capacity bytes; sc_nearest_release gives them back.
 */
#define SC_RADIUS_LDS_ROW 1024 /* the longest row sorted in LDS: 12 KiB per wavefront, 48 KiB per block */
int sc_radius(const double *queries, int queries_on_device, int64_t Q,
              const double *targets, int targets_on_device, int64_t P,
              double radius, int device,
              int32_t *counts_out /* [Q] or NULL */, int64_t *offsets_out /* [Q + 1] or NULL */,
              int32_t *index_out, double *d2_out, int64_t capacity /* both or neither */,
              int out_on_device /* where the four arrays above live */,
              int64_t *total_out /* host, required */,
              int64_t *long_out /* host, optional: rows the long-row launch sorted */,
              void *hip_stream);

/*
 * Graph distances to a root and connected components: the two graph steps of the reference's XU
 * skeleton (plant3dvision/proc3d.py:212-426) -- nx.dijkstra_predecessor_and_distance(g, root)'s distances and
 * nx.connected_components, of the whole graph or of the nodes of one key -- over the rows sc_knn and sc_radius return,
 * on the GPU.  The distances are PINNED: a label-correcting fixpoint in float64 gives Dijkstra's numbers bit for bit
 * (tests/test_graph_host.py compares with networkx and scipy).
 *
 * The graph: N nodes and rows of arcs, in one of two forms --
 *   CSR:          offsets int64 [N + 1], index int32 [E]            (sc_radius of a cloud against itself);
 *   fixed length: offsets == NULL, row_len = k, index int32 [N][k], -1 in unused places, E = N * k   (sc_knn);
 * then M extra pairs, extra int32 [M][2] with extra_w double [M] (plain weights), which may be NULL with M == 0.  All
 * arrays, the outputs among them, live on the host or on the device as on_device says; device arrays are read in place
 * on the given stream.
 *   G1. every arc (i, j, w) with j != i is an undirected edge, usable in both directions (knn rows are not symmetric,
 *       the reference's nx.Graph is).  Self-arcs and repeated arcs change nothing.  weights double [E] are taken as
 *       they are, or with weights_squared as sqrt of the given d2: computed on the device in float64, correctly rounded;
 *   G2. sc_graph_distances: d[root] = +0.0; d[v] is the least, over all walks root = v0 .. vm = v, of the left-to-right
 *       float64 sum ((0 + w1) + w2) + ..; +inf where no walk exists.  This is what Dijkstra with a float64 accumulator
 *       returns.  dist_out double [N].  rounds_out: NULL, or one host int64 that receives the number of rounds run.  The
 *       call always ends in a wait (the rounds are counted on the host, SC_GRAPH_ROUNDS_PER_WAIT between two looks);
 *   G3. sc_graph_components: without a key label[v] is the rank of v's component when components are ordered by their
 *       smallest member (sc_dbscan's numbering).  With key int32 [N] an edge joins its ends only where
 *       key[i] == key[j] >= 0; nodes with key < 0 get label -1 and arcs to them are ignored.  labels_out int32 [N];
 *       ncomponents_out: NULL, or one host int32 (the call then ends in a wait, as it does with host arrays);
 *   G4. refused (SC_ERR_INVALID, before the first device call for host arrays; for device arrays by a first kernel
 *       that only judges, as sc_nearest does for coordinates): an index outside -1 .. N - 1 (-1 only in the fixed-length
 *       form; an extra pair outside 0 .. N - 1), offsets that do not rise from 0 to E, weights that are NaN, negative or
 *       infinite (places holding -1 are not looked at), root outside 0 .. N - 1, N, E or E + M outside 0 .. 2^31 - 1,
 *       E != N * row_len in the fixed-length form, NULL arrays, the device ordinal.  N == 0 makes no device call.
 * The frontier loop runs at most N rounds (a lowering walk has fewer than N arcs); a frontier left after that is
 * SC_ERR_DEVICE.  Work buffers (the adjacency at 12 bytes per directed arc, two frontiers, stamps, scan storage; copies
 * of host arrays) are kept per device between calls while they are at most 1 GiB, ordered across streams as
 * sc_dbscan's are, and given back by sc_graph_release.  Errors are read with sc_graph_error (the unit's own last
 * message).  sc_graph_set_blocks caps every grid of the unit, 0 restores the default: tests drive the grid-stride loops
 * past their first trip with it; no answer depends on it.
 */
#define SC_GRAPH_ROUNDS_PER_WAIT 64
int sc_graph_distances(int64_t N, const int64_t *offsets /* [N + 1] or NULL */, int row_len, const int32_t *index /* [E] */,
                       const double *weights /* [E] */, int64_t E, int weights_squared,
                       const int32_t *extra /* [M, 2] */, const double *extra_w /* [M] */, int64_t M,
                       int on_device /* where every array and dist_out live */, int64_t root, int device,
                       double *dist_out /* [N] */, int64_t *rounds_out /* host, may be null */, void *hip_stream);
int sc_graph_components(int64_t N, const int64_t *offsets /* [N + 1] or NULL */, int row_len, const int32_t *index /* [E] */, int64_t E,
                        const int32_t *extra /* [M, 2] */, int64_t M, const int32_t *key /* [N] or NULL */,
                        int on_device /* where every array and labels_out live */, int device,
                        int32_t *labels_out /* [N] */, int32_t *ncomponents_out /* host, may be null */, void *hip_stream);
/*
 * The quotient of the graph under a labelling: what the XU skeleton needs behind the components -- the
 * clusters renumbered, their member counts and centres, and nx.quotient_graph's edges with their weights -- on the GPU.
 * The graph, the extra pairs, on_device (one flag for every array and output), the slots, the error getter and the grid
 * cap are sc_graph_distances'.  labels int32 [N] name a label 0 .. L - 1 per node, key int32 [N] (or NULL) and points
 * double [N][3] (or NULL) belong to the nodes.
 *   Q1. clusters: a node with labels[v] < 0 is outside: cluster_out[v] = -1, and arcs to it are ignored.  A label with
 *       no member gets no cluster.  The labels that have members are ordered by (kmin, smallest): kmin the least key
 *       over the label's members (signed compare; 0 without a key), smallest its least member.  cluster is the rank in
 *       that order, C the number of such labels.  With G3's labels and key = the bins this is "numbered by (bin,
 *       smallest member)"; without a key it is G3's numbering.  cluster_out int32 [N];
 *   Q2. centres: counts_out[c] is the number of members; centers_out[c][a] is s / (double)counts[c], where s starts at
 *       +0.0 and adds points[v][a] over the members in rising v, left to right in float64; the division is correctly
 *       rounded.  This is np.bincount(cluster, weights=...) / count bit for bit.  Points are not judged: NaN and
 *       infinities flow through as they do in NumPy.  counts_out int32 [L], centers_out double [L][3] (may be NULL
 *       when points is NULL); rows C .. L - 1 of both are left untouched;
 *   Q3. cluster edges: the pairs (a < b) of distinct clusters for which some arc, of the rows or extra and in either
 *       direction, joins a member of a with a member of b; sorted lexicographically, K of them.  edges_out int32
 *       [capacity][2];
 *   Q4. weights: first the arcs fold into undirected node edges: every unordered node pair {i < j} with at least one arc
 *       gets w{i,j}, the least of its arcs' weights (by G1 the square root of d2 when weights_squared; under N1 d2 is
 *       bitwise symmetric, so for knn and radius rows all arcs of a pair agree, and the minimum makes the rule
 *       order-free for anything else).  edge_w_out[e] starts at +0.0 and adds w{i,j} over the node pairs that join the
 *       two clusters, in rising (i, j), left to right: the `weight` of nx.quotient_graph up to summation order.
 *       edge_w_out double [capacity] or NULL; weights and extra_w may be NULL when it is NULL;
 *   Q5. capacity is sc_radius's R6: the call always computes C, K, cluster_out, the counts and the centres; it writes
 *       edges_out / edge_w_out iff capacity >= K, otherwise it returns SC_OK with *nedges_out = K and leaves them
 *       untouched;
 *   Q6. refused (SC_ERR_INVALID): what G4 refuses, the weights judged only when edge_w_out is given; L outside 0 .. N;
 *       a label >= L (host arrays before the first device call, device arrays by the judging kernel); NULL labels,
 *       cluster_out, counts_out (with L > 0), centers_out with points (with L > 0), nclusters_out or nedges_out; a
 *       negative capacity, or a positive one with NULL edges_out; edge_w_out without edges_out, without weights (E > 0)
 *       or without extra_w (M > 0).  N == 0 makes no device call and gives C = K = 0.
 * nclusters_out (host int32) and nedges_out (host int64) are required, so the call ends in a wait.  Waits in all: with
 * device arrays three (the judge's flag; C and the number of crossing arcs, which size the sorts; K), with host arrays
 * two (the last two) and one more when edge rows go home.  No floating-point atomic: every sum has the one order of its
 * rule.  Work buffers, on the slots as above: per label 48 bytes; per node, when centres are asked for, 40 bytes; per
 * arc (E + M places) 24 bytes, 40 with weights; scan and sort storage; copies of host arrays and of host outputs.
 */
int sc_graph_quotient(int64_t N, const int64_t *offsets /* [N + 1] or NULL */, int row_len, const int32_t *index /* [E] */,
                      const double *weights /* [E] or NULL */, int64_t E, int weights_squared,
                      const int32_t *extra /* [M, 2] */, const double *extra_w /* [M] or NULL */, int64_t M,
                      const int32_t *labels /* [N] */, int64_t L, const int32_t *key /* [N] or NULL */,
                      const double *points /* [N, 3] or NULL */, int on_device /* where every array and output lives */, int device,
                      int32_t *cluster_out /* [N] */, int32_t *counts_out /* [L] */, double *centers_out /* [L, 3] or NULL */,
                      int32_t *edges_out /* [capacity, 2] */, double *edge_w_out /* [capacity] or NULL */, int64_t capacity,
                      int32_t *nclusters_out /* host */, int64_t *nedges_out /* host */, void *hip_stream);
/*
 * The edges that connect the labels of a cloud to the root's: what the reference's connect_graph
 * (plant3dvision/proc3d.py:212-263) adds to a graph to make it connected, in an order-free form, on the GPU.  It is
 * Prim's algorithm over the labels, started at the root's.  points double [N][3], labels int32 [N] (sc_graph_components'
 * labels_out, or any other labelling), L the label bound.  on_device (one flag for every array and output), the slots,
 * the error getter and the grid cap are sc_graph_distances'.
 *   C1. the set and the rounds: R starts as the nodes whose label is labels[root].  While a node lies outside R, the
 *       pair (i not in R, j in R) with the least key (d2, i, j), compared lexicographically, becomes edge number m,
 *       stored as edges_out[m] = (i, j) with weights_out[m] = sqrt(d2), and every node with labels[i]'s label joins R.
 *       d2 is rule N1's ((dx dx) + (dy dy)) + (dz dz) in binary64 without contraction, bitwise symmetric; the square
 *       root is correctly rounded (G1).  *nedges_out is the number of labels that have members, minus one; places of
 *       edges_out int32 [L - 1][2] and weights_out double [L - 1] behind that count stay untouched;
 *   C2. labels need not be components: any labelling 0 .. L - 1 is taken as given, labels without members are allowed.
 *       Nothing depends on how members are ordered inside a label: ties are decided by the key (d2, i, j), never by
 *       the order in which anything arrives;
 *   C3. refused (SC_ERR_INVALID): N outside 0 .. 2^31 - 1; L outside 1 .. N (for N > 0); a label outside 0 .. L - 1; a
 *       root outside 0 .. N - 1; a non-finite coordinate (as N5 refuses them); NULL points, labels or nedges_out; NULL
 *       edges_out or weights_out when L > 1; the device ordinal.  Host arrays are judged before the first device call;
 *       device arrays by a first kernel that only judges and reads labels[0 .. N) and points[0 .. 3 N) and nothing
 *       else, and the entry waits for its flag before any other launch.  N == 0 makes no device call and gives
 *       *nedges_out = 0;
 *   C4. bounds: every loop has a bound fixed before it starts; no wavefront waits on another, no kernel persists or
 *       spins, there is no floating-point atomic; blocks meet only at kernel boundaries (and in the integer counters
 *       that lay the points out in label order, where C2 makes the order irrelevant).  One launch per round: round 0
 *       lets the root's label join, round r > 0 writes edge r - 1.  min(SC_GRAPH_ROUNDS_PER_WAIT, L) rounds are
 *       enqueued, then the entry waits and reads C, the number of labels with members; the C - 1 - (rounds run) that
 *       remain are enqueued in one go and waited for.  A round behind the last edge, or one that finds nobody outside,
 *       returns at once.  Labels left outside after L - 1 edge rounds are SC_ERR_DEVICE.  Waits in all: the judge's
 *       (device arrays only), one after the first rounds, one after the rest (device arrays: only when rounds remain;
 *       host arrays with C > 1: always, the edges go home in front of it);
 *   C5. work buffers, on the slots as above and under the same 1 GiB keep policy: per node 40 bytes (the coordinates
 *       and the index in label order, the best (d2, j)); per label 12 bytes; 32 bytes per block of the grid; scan
 *       storage; for host arrays copies of points and labels (28 bytes per node) and of the outputs (16 per label).
 * Work is at most N^2 / 2 evaluations of d2 however many labels there are: a node is offered every other node once.
 */
int sc_graph_connect(int64_t N, const double *points /* [N, 3] */, const int32_t *labels /* [N] */, int64_t L, int64_t root,
                     int on_device /* where every array and output lives */, int device,
                     int32_t *edges_out /* [L - 1, 2] */, double *weights_out /* [L - 1] */, int64_t *nedges_out /* host */,
                     void *hip_stream);
const char *sc_graph_error(void);
void sc_graph_release(void);
void sc_graph_set_blocks(int blocks);

/* Page-locked host memory for the read-back of sc_get_values (no reference counterpart: the
 * reference's values_h is a pageable NumPy array, cl.py:173).  A 512 MiB volume reads back in
 * ~10 ms into such a buffer against ~50 ms into pageable memory, but allocating it takes ~0.1 s
 * during which other threads' HIP calls stall (measured: doing it on a thread beside the mask
 * ingest made a one-shot run slower), so it only pays for callers that keep the buffer across
 * many read-backs.  sc_host_free needs no engine: the buffer may outlive it. */
int sc_host_alloc(int device, int64_t bytes, void **ptr);
void sc_host_free(void *ptr);

/* Device-memory helpers so that hosts without a HIP binding can stage inputs in HBM
 * (bench.py, tests): plain hipMalloc / hipMemcpy / hipFree on the engine's device. */
int sc_dev_alloc(sc_engine *e, int64_t bytes, void **ptr);
int sc_dev_free(sc_engine *e, void *ptr);
int sc_dev_upload(sc_engine *e, void *dst_dev, const void *src_host, int64_t bytes);
int sc_dev_download(sc_engine *e, void *dst_host, const void *src_dev, int64_t bytes);

/*
 * Mask ingest (cl.py:298, `io.read_image`): decoder for 8-bit greyscale, non-interlaced PNG -- the files a
 * `Masks` / `Segmentation2D` fileset holds -- callable from the decode-ahead threads with the interpreter
 * lock released (the Python decoders stop scaling at ~3 threads).  sc_png_info returns SC_OK and the
 * size for a file this decoder takes, SC_ERR_INVALID (reason: sc_png_last_error) for anything else
 * (other colour types, bit depths, interlacing, palette or transparency chunks): the caller then uses
 * its usual reader.  sc_png_decode_gray8 writes H*W bytes, row-major.  Host code only (zlib).
 */
int sc_png_info(const void *data, int64_t len, int *W, int *H);
int sc_png_decode_gray8(const void *data, int64_t len, uint8_t *out, int W, int H);
const char *sc_png_last_error(void);

/*
 * Several GPUs from ONE process (SURVEY.md 8b `sc_create_sharded`; the reference drives a single
 * device, cl.py:29-30): one engine per entry of `devices` (HIP ordinals; an ordinal may repeat), the
 * x-planes of the grid dealt round-robin over them (partition 0; every device then holds the same share
 * of the object) or in contiguous slabs (partition 1), voxel coordinates from the GLOBAL plane index as
 * in sc_create_cyclic / sc_create_slab.  Every view goes to every engine; sc_group_get_values writes
 * the whole [nx][ny][nz] grid in global order (one strided device-to-host copy per device).  The
 * one-process-per-GPU form of the same sharding is plant-3d-vision_amd/sharded.py over RCCL.
 * A view's arguments are judged once, before any engine takes it.  Should a call still fail on some engine
 * after others took it (a device error), the planes are in different states: the group then answers
 * SC_ERR_STATE to everything but sc_group_clear (every engine back to default_value) and sc_group_destroy.
 */
typedef struct sc_group sc_group;
int sc_create_sharded(sc_group **out, int64_t nx, int64_t ny, int64_t nz, const float origin[3],
                      float voxel_size, int mode, float default_value, const int *devices, int ndev,
                      int partition);
void sc_group_destroy(sc_group *g);
int sc_group_size(const sc_group *g);
sc_engine *sc_group_engine(sc_group *g, int i);  /* for per-engine calls (options, statistics, device batches) */
int sc_group_clear(sc_group *g);
int sc_group_set_option(sc_group *g, int key, int64_t value);
int sc_group_set_lut(sc_group *g, const float *lut256);
int sc_group_process_view(sc_group *g, const float K[4], const float R[9], const float t[3], const void *mask,
                          int H, int W, int mask_dtype, int64_t row_stride_bytes);
int sc_group_flush(sc_group *g);
int sc_group_synchronize(sc_group *g);
int sc_group_get_values(sc_group *g, void *out);

#ifdef __cplusplus
}
#endif
#include "spacecarve_tuning.h" /* the SC_OPT_* tuning keys: same key space, results never depend on them */
#endif /* SPACECARVE_H */
