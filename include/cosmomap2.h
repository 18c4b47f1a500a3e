/*
 * cosmomap2.h -- C ABI of libcosmomap2_hip.so, the MI355X (gfx950) implementation
 * of the COSMOMAP2 PCG map-making hot path.
 *
 * The reference (giuspugl/COSMOMAP2) has no FFI of its own: its native code is a
 * set of C++ loop bodies held as Python strings and JIT-compiled by weave.inline
 * (e.g. interfaces/linearoperators.py:368-382).  Each entry point below replaces
 * one of those loops (or the NumPy/BLAS lines that play the same role) and cites
 * it.  The Python binding a maintainer would add in place of each
 * `inline(code, ...)` call is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure: CM2_ERR_HIP (1) a HIP runtime call
 *     failed, CM2_ERR_ARGUMENT (2) an argument or the state of an object was refused, CM2_ERR_OUT_OF_MEMORY
 *     (3) a device allocation failed even after the library gave back its own cached blocks -- the one
 *     failure a host may answer by freeing device memory of its own and calling again, PROVIDED the entry
 *     point overwrites its outputs (every *_create, *_prepare_*, *_apply; not the in-place updates
 *     cm2_axpy, cm2_scal, cm2_Z_axpy, cm2_panel_gemm(accumulate), cm2_pcg_update_*, cm2_flag_samples, nor
 *     the drivers cm2_pcg, cm2_pcg_sharded, cm2_arnoldi);
 *     cm2_last_error() returns a static, thread-local message for the last failure;
 *   - pointers named d_* are DEVICE pointers, h_* are HOST pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work
 *     is enqueued on it and the call returns without synchronising unless stated;
 *   - maps are pixel-interleaved doubles [I0,Q0,U0,I1,...] (linearoperators.py:487);
 *     pixel ids are int32, -1 marks a flagged sample (linearoperators.py:372);
 *     all arithmetic is IEEE double, no FMA contraction, reference operand order;
 *   - one context per process per GPU.  Objects may be shared by host threads for APPLICATION
 *     calls once their lazily built parts exist (cm2_tiles_prepare_pt, cm2_noise_prepare_tiles,
 *     cm2_pointing_build_sell); construction and destruction are not thread-safe (the reference is
 *     single-threaded).  Exception: a tile plan whose P^T uses scratch of the plan (tiles
 *     split over workgroups on an uneven hit map, hot one-pixel tiles: cm2_tiles_pt_parts reports
 *     both as "tiles split" / copy bytes > 0) must not run two P^T applications at the same time on
 *     different streams; applications on one stream, or of different plans, are fine.
 */
#ifndef COSMOMAP2_H
#define COSMOMAP2_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): cm2_noise_prepare_tiles, cm2_set_exact_order, cm2_pcg_sharded and cm2_tiles_pt_parts added;
 * uneven hit maps keep uniform tiles and split the heavy ones over workgroups (cm2_tiles_pixel_range); cm2_noise_tile_kernel_info reports the one-real-window
 * kernel only; and the defaults that changed behind unchanged signatures since version 1 --
 * cm2_pointing_info fields 3..5 are -1 until the pixel-major copy exists, cm2_tiles_set_pt_order has
 * mode 2 and its default sums runs of more than 256 hits per slice in chunks of 32 terms,
 * cm2_weights_accumulate sums pixels with >= 8192 samples in chunks (both <= 1e-14 from the serial
 * sum; CM2_PT_ORDER=exact / CM2_WEIGHTS_ORDER=exact or cm2_set_exact_order(1) restore the serial
 * order), cm2_pcg calls its callback after the next iteration's work is queued. */
#define CM2_ABI_VERSION 2
/* status codes (added in round 5 behind the same "non-zero on failure" contract: no version change) */
#define CM2_ERR_HIP 1
#define CM2_ERR_ARGUMENT 2
#define CM2_ERR_OUT_OF_MEMORY 3

const char *cm2_last_error(void);
int cm2_abi_version(void);
/* device properties used by the bench harness (name buffer >= 256 bytes) */
int cm2_device_info(int device, char *h_name, int *h_num_cu, double *h_hbm_gib);
/* Device memory of the library.  Every buffer a cm2_* object owns and every temporary of a plan
 * build comes from a per-device cache of released blocks (a released block is handed out again to
 * a request of at most 25 % less; releasing waits for the device exactly like hipFree).  The cache
 * holds at most CM2_DEVICE_CACHE_MB megabytes (environment; default: an eighth of the device's memory,
 * 36 GB on an MI355X; 0 = every release goes straight back to the driver).  Other allocators on the
 * same device (the host framework's, another rank's) do not see these blocks: a host that runs out of
 * device memory should call cm2_release_cached_memory and retry (cosmomap2_amd/device.py does).  cm2_release_cached_memory returns all cached blocks to the
 * driver; cm2_device_memory_info fills h_info[4] = bytes in use by live objects, bytes cached,
 * requests served from the cache, requests that went to the driver. */
int cm2_release_cached_memory(void);
/* Summation order of the per-pixel sums (process-wide; objects created afterwards follow it).  The
 * reference adds every pixel's terms serially in time order (linearoperators.py:509-516,
 * process_ces.py:426-555).  Default (on = 0): that order, except that a pixel with >= 8192 samples
 * (weights) or a run of more than 256 hits inside one slice of a tile (P^T) is summed in fixed chunks
 * -- reproducible, independent of the rest of the hit map, <= 1e-14 relative from the serial sum, so
 * a pixel whose condition number sits within 1e-14 of threshold_cond (process_ces.py:544-550) could
 * be masked differently.  on = 1: the pure serial order everywhere (bit-equal to the reference's
 * loops; a stare at one pixel then costs milliseconds to seconds).  on = -1: back to the environment
 * (CM2_PT_ORDER, CM2_WEIGHTS_ORDER). */
int cm2_set_exact_order(int on);
int cm2_device_memory_info(int64_t *h_info);

/* ------------------------------------------------------------------------- *
 * a1-a3  Pointing matrix  (SparseLO, interfaces/linearoperators.py:326-557)
 * ------------------------------------------------------------------------- */
typedef struct cm2_pointing cm2_pointing;

/* Builds the device-side pointing plan from time-ordered arrays that are
 * already resident in HBM.  The plan KEEPS the three pointers (caller keeps the
 * buffers alive) and adds a pixel-major copy: samples grouped by pixel in time
 * order, 64 pixels per slice, slices sorted by hit count (sliced-ELL), which is
 * what makes P^T a race-free, fixed-order reduction (built lazily, see LIFETIME below).
 * d_cos/d_sin may be NULL for pol == 1.  Replaces SparseLO.__init__
 * (linearoperators.py:527-550); pol not in {1,2,3} fails like the RuntimeError at :549.
 * Synchronises. */
int cm2_pointing_create(cm2_pointing **out, const int32_t *d_pix, const double *d_cos,
                        const double *d_sin, int64_t nt, int64_t npix, int pol,
                        void *stream);
int cm2_pointing_destroy(cm2_pointing *p);
/* LIFETIME: the pixel-major copy is built by its first user (cm2_Pt_apply, cm2_pointing_set_weights,
 * cm2_PtNP_diag_apply) or by cm2_pointing_build_sell, FROM d_pix / d_cos / d_sin: the caller must keep
 * those three buffers alive AND UNCHANGED at least until then (cm2_P_apply reads them for the whole
 * life of the plan).  An operator that only runs on the tile order (cm2_tiles) never builds it. */
int cm2_pointing_build_sell(cm2_pointing *p, void *stream);
/* h_info[0..5] = nt, npix, pol, then valid samples, padded pixel-major length, slices of the
 * pixel-major copy, or -1, -1, -1 while that copy has not been built (this call builds nothing) */
int cm2_pointing_info(const cm2_pointing *p, int64_t *h_info);

/* P x: gather, time order.  d_out[t] = I_p + Q_p cos2phi_t + U_p sin2phi_t, 0 for
 * flagged samples.  Replaces the weave loops at linearoperators.py:368-375
 * (mult), :424-430 (mult_qu), :483-489 (mult_iqu). */
int cm2_P_apply(const cm2_pointing *p, const double *d_x, double *d_out, void *stream);

/* P^T v: scatter-add in sample order per pixel, written as a per-pixel
 * fixed-order reduction.  Replaces linearoperators.py:394-400 (rmult),
 * :447-454 (rmult_qu), :509-516 (rmult_iqu).  Overwrites d_out (pol*npix). */
int cm2_Pt_apply(const cm2_pointing *p, const double *d_v, double *d_out, void *stream);

/* Attach per-sample diagonal noise weights w_t = (N^-1)_tt (time order, nt
 * doubles; NULL = all ones) for the fused matvec below.  Replaces the role of
 * BlockLO.diag (linearoperators.py:677-683). */
int cm2_pointing_set_weights(cm2_pointing *p, const double *d_w, void *stream);

/* Fused P^T diag(w) P x in ONE pass over the pixel-major samples; no TOD vector
 * is materialised.  Same arithmetic, in the same order, as the reference's
 * three-stage chain (P.T*N*P)*x  (tests/test_toeplitz_vector_multiplication.py:24-28,
 * call stack SURVEY 3.2). */
int cm2_PtNP_diag_apply(const cm2_pointing *p, const double *d_x, double *d_out,
                        void *stream);

/* ------------------------------------------------------------------------- *
 * a2-a3 (throughput form)  Tile-bucketed TOD order
 *   Samples grouped by pixel tile (stable, so time order inside a tile); the tile's
 *   slice of the map is staged in LDS, so P and P^T stream HBM with no random access.
 *   The order is internal: TB-ordered TODs are only ever produced and consumed by the entry points of
 *   this section and cm2_noise_apply_tiles / cm2_filter_apply_tiles.
 *   Same loops as above (linearoperators.py:483-489, :509-516).  P^T by default adds every
 *   pixel's terms in time order from 0 like the serial loop (one workgroup per tile, per-slice
 *   lists sorted by (pixel, time), no atomics: bitwise reproducible); cm2_tiles_set_pt_order(t, 0)
 *   or CM2_PT_ORDER=atomic selects LDS + global fp64 atomics (term order not fixed).
 * ------------------------------------------------------------------------- */
typedef struct cm2_tiles cm2_tiles;
int cm2_tiles_create(cm2_tiles **out, const int32_t *d_pix, const double *d_cos,
                     const double *d_sin, int64_t nt, int64_t npix, int pol, int tile_pixels,
                     int64_t slice_samples, void *stream);
int cm2_tiles_destroy(cm2_tiles *t);
/* h_info[0..11] = nt, valid samples (= length of a TB-ordered TOD), tile pixels, tiles, items,
 * 1 if the plan stores one half-angle value per sample instead of cos and sin (done when every
 * (cos, sin) pair is on the unit circle to 1e-14; the kernels rebuild cos = +-(1-h^2)/(1+h^2),
 * sin = 2h/(1+h^2), absolute error <= 3.4e-16, and read 8 bytes less per sample), 1 if P^T sums in
 * fixed (time) order, the plan's id (unique per plan in this process), slice length of the
 * fixed-order lists (0 until the first P^T builds them), the bytes one fixed-order P^T is
 * designed to read (TOD + padded lists), then 1 and the padded sample count (the two fields of the
 * span order removed in round 5: one span = the global tile order) */
int cm2_tiles_info(const cm2_tiles *t, int64_t *h_info);
/* fixed == 1 (default): P^T adds each pixel's terms in time order (the reference's order,
 * reproducible bit for bit), except that a pixel hit more than 256 times inside one slice of a
 * tile's samples (hot pixels: a stare at a source) is summed in chunks of 32 consecutive terms
 * whose sums are then added in time order -- a fixed regrouping, still reproducible bit for bit
 * and independent of the hit map, ~1e-16 relative away from the serial sum;
 * fixed == 2 ("exact", CM2_PT_ORDER=exact): pure time order for every pixel whatever its hit count
 * (one thread walks a hot run: 1e5 hits in one pixel cost milliseconds);
 * fixed == 0 (CM2_PT_ORDER=atomic): LDS / global atomics, term order not fixed */
int cm2_tiles_set_pt_order(cm2_tiles *t, int fixed);
/* Builds the per-slice (pixel, time) lists of the fixed-order P^T now (allocations, sorts, one
 * synchronisation) instead of inside the first cm2_Pt_tiles_apply: afterwards an application only
 * launches kernels, so it may be captured into a graph or issued from several host threads.  A plan
 * that was not prepared builds the lists on its first P^T under a lock.  No-op for the atomic form. */
int cm2_tiles_prepare_pt(cm2_tiles *t, void *stream);
/* Work items of the fixed-order P^T after cm2_tiles_prepare_pt: h_info[0..3] = workgroups per
 * application (= tiles when no tile is split), tiles that are split, bytes of the plan's P^T scratch
 * (tile copies of the split tiles, range sums of hot one-pixel tiles), and
 * 1000 x (simulated finish time of the items on two resident workgroups per CU / ideal). */
int cm2_tiles_pt_parts(const cm2_tiles *t, int64_t *h_info);
/* h_p0p1[0..1] = pixel range [p0, p1) covered by the tiles [tile_lo, tile_hi).  Tiles are uniform
 * (tile_pixels wide).  On an uneven hit map (a uniform tile holding over 25 % more samples than the
 * mean) the fixed-order P^T shares the slices of the heavy tiles out to several workgroups, each
 * summing consecutive slices in time order into its own copy of the tile, and adds the copies in time
 * order: a fixed regrouping of the serial sum (part boundaries depend on the plan only: reproducible
 * bit for bit; ~1e-16 relative away from the serial sum); a pixel with at least 32768 samples and half
 * a tile's mean load becomes a one-pixel tile of its own (summed as described at
 * cm2_tiles_set_pt_order).  CM2_TILE_BALANCE: 0 = uniform tiles, one workgroup each; 1 / cut = pixel
 * ranges re-cut to equal sample counts (never wider than tile_pixels), one workgroup each -- the same
 * bits as the uniform tiling, chosen automatically when the exact order is asked for
 * (cm2_set_exact_order, CM2_PT_ORDER=exact); parts = the default on uneven maps, forced. */
int cm2_tiles_pixel_range(const cm2_tiles *t, int64_t tile_lo, int64_t tile_hi, int64_t *h_p0p1);
/* h_tiles[0..ngroups]: group g = tiles [h_tiles[g], h_tiles[g+1]) -- consecutive pieces of the map
 * for cm2_Pt_tiles_apply_range whose pixel boundaries depend on npix and tile_pixels only, so that
 * every rank of a TOD-sharded run reduces the same pixels (balanced tilings keep these cuts). */
int cm2_tiles_group_tiles(const cm2_tiles *t, int ngroups, int64_t *h_tiles);
/* d_tod_tb[k] = (P x) for the k-th sample in TB order */
int cm2_P_tiles_apply(const cm2_tiles *t, const double *d_x, double *d_tod_tb, void *stream);
/* d_out = P^T v for a TB-ordered v (d_out is overwritten) */
int cm2_Pt_tiles_apply(const cm2_tiles *t, const double *d_tod_tb, double *d_out, void *stream);
/* integer per-sample labels (e.g. ground bins) from time order to TB order; set-up use */
int cm2_i32_time_to_tiles(const cm2_tiles *t, const int32_t *d_time, int32_t *d_tb, void *stream);
/* P^T restricted to the tiles [tile_lo, tile_hi): overwrites the entries of d_out that belong to
 * those tiles (pixels tile_lo*tile_pixels .. min(tile_hi*tile_pixels, npix)) and nothing else, so
 * that a finished part of the map can be reduced across GPUs while the next part is computed. */
int cm2_Pt_tiles_apply_range(const cm2_tiles *t, const double *d_tod_tb, double *d_out,
                             int64_t tile_lo, int64_t tile_hi, void *stream);
/* permutations between time order (nt, flagged samples read as / written with 0) and TB order */
int cm2_tod_time_to_tiles(const cm2_tiles *t, const double *d_time, double *d_tb, void *stream);
int cm2_tod_tiles_to_time(const cm2_tiles *t, const double *d_tb, double *d_time, void *stream);

/* ------------------------------------------------------------------------- *
 * a4-a5  Noise operator N^-1  (ToeplitzLO linearoperators.py:560-602,
 *        BlockLO :627-697, blk_matvec interfaces/blkop.py:178-208)
 * ------------------------------------------------------------------------- */
typedef struct cm2_noise cm2_noise;

#define CM2_TOEPLITZ_AUTO   0   /* direct for short bands, fused FFT, rocFFT beyond its range */
#define CM2_TOEPLITZ_DIRECT 1   /* O(n*lambda), reference summation order  */
#define CM2_TOEPLITZ_FFT    2   /* overlap-save, rocFFT R2C/C2R fp64       */
#define CM2_TOEPLITZ_FUSED  3   /* overlap-save, one kernel, fp64 FFT in LDS (lambda <= 2049) */

/* Block-diagonal with constant diagonal blocks: block b = h_t[b] * I of
 * h_sizes[b] samples (BlockLO offdiag=False, :676-683). */
int cm2_noise_create_diag(cm2_noise **out, const double *h_t, const int64_t *h_sizes,
                          int64_t nblocks);
/* Block-diagonal of symmetric banded Toeplitz blocks: block b has first row
 * h_bands[b*lambda .. b*lambda+lambda-1] (ToeplitzLO.mult :582-595), zero
 * boundary at each block edge -- never circulant, never across blocks. */
int cm2_noise_create_toeplitz(cm2_noise **out, const double *h_bands, int64_t lambda,
                              const int64_t *h_sizes, int64_t nblocks, int method,
                              void *stream);
int cm2_noise_destroy(cm2_noise *n);
/* y = N^-1 v over all blocks (blk_matvec, blkop.py:195-206).  d_out != d_v.  Nothing is built on the
 * first application: the create call leaves the state of every method complete. */
int cm2_noise_apply(cm2_noise *n, const double *d_v, double *d_out, void *stream);
/* y = N^-1 v with v and y both in the tile-bucketed order of `tiles` (CM2_TOEPLITZ_FUSED
 * operators, and CM2_TOEPLITZ_AUTO ones with lambda <= 2049): the permutation to and from time order
 * is folded into the overlap-save kernel's own loads and stores (ToeplitzLO.mult :582-595 per block,
 * blkop.py:195-206).  d_out_tb != d_in_tb.
 * cm2_noise_prepare_tiles builds the address lists of the (operator, tile plan) pair: it allocates,
 * launches the list builders on `stream` and WAITS for them.  After it, cm2_noise_apply_tiles for the
 * same plan is one kernel launch -- no allocation, no synchronisation, safe inside a stream capture
 * and from several host threads.  Without it the first application prepares the lists itself (under
 * the operator's lock).  An operator keeps the lists of its three most recently used tile plans. */
int cm2_noise_prepare_tiles(cm2_noise *n, const cm2_tiles *tiles, void *stream);
int cm2_noise_apply_tiles(cm2_noise *n, const cm2_tiles *tiles, const double *d_in_tb,
                          double *d_out_tb, void *stream);
/* y = P^T N^-1 P x in ONE call on the tile order (the chain `P.T*N*P` of the reference's scripts,
 * src/test_M2_precond_onto_real_data.py:79-86, SURVEY 8b's cm2_PtNP_apply): cm2_P_tiles_apply,
 * cm2_noise_apply_tiles, cm2_Pt_tiles_apply on `stream`.  d_tb1 != d_tb2: scratch of at least
 * (valid samples of the plan, cm2_tiles_info[1]) doubles each. */
int cm2_PtNP_tiles_apply(const cm2_tiles *tiles, cm2_noise *n, const double *d_x, double *d_y,
                         double *d_tb1, double *d_tb2, void *stream);
/* per-sample diagonal of a constant-diagonal noise operator (BlockLO.diag). */
int cm2_noise_expand_diag(const cm2_noise *n, double *d_w, void *stream);
/* h_info[0..5] = nt, nblocks, lambda (0 for diag), method used, FFT length, 1 if
 * cm2_noise_apply_tiles is available (CM2_TOEPLITZ_FUSED, or CM2_TOEPLITZ_AUTO with lambda <= 2049:
 * an AUTO operator that applies the direct sum on the time order still runs the fused
 * overlap-save kernel on a tile order) */
int cm2_noise_info(const cm2_noise *n, int64_t *h_info);
/* What cm2_noise_apply_tiles runs for this operator (none of this exists in the reference, whose
 * ToeplitzLO.mult is a NumPy loop, interfaces/linearoperators.py:582-595): h_info[0] = complex points
 * per thread of the one-real-window kernel (32), h_info[1] = list format of the most recently used
 * tile plan (1 plain, 2 run-coded lists cut by time, 3 run-coded lists cut by address ("inverse"),
 * 0 = no lists built yet), h_info[2] = window length in samples, h_info[3] = 0 (was: windows across
 * two spans of the span order removed in round 5);
 * *h_bytes_per_sample = HBM bytes per TOD sample the kernel is built to move (lists + gathered windows +
 * results).  Environment switches,
 * read ONCE when the operator is created: CM2_OS_LISTS = auto (default: rc below 768 pixel tiles,
 * inv from there up) | rc | inv | plain, CM2_OS_LIST_BUILD = direct (default) | sort, CM2_OS_FLAT
 * (flat addressing also for buffers below 4 GB). */
int cm2_noise_tile_kernel_info(const cm2_noise *n, int64_t *h_info, double *h_bytes_per_sample);

/* ------------------------------------------------------------------------- *
 * a6-a7  ProcessTimeSamples  (utilities/process_ces.py:58-555)
 * ------------------------------------------------------------------------- */
/* Per-pixel sums of w, w c, w s, w c c, w s s, w s c over the samples of each
 * pixel IN TIME ORDER (fixed-order, race-free).  pol=1 fills d_counts only,
 * pol=2 the last three, pol=3 all six (unused outputs may be NULL).  d_w NULL =
 * ones (process_ces.py:65-66).  Replaces :480-487, :505-514, :527-539 and
 * compute_arrays :125-186.  Synchronises (builds a temporary pixel index).
 * A pixel with 8192 samples or more (a stare at a source; one thread would walk
 * 5e6 samples for 1.9 s) is summed in fixed chunks of 4096 samples -- 256 strided
 * partial sums, a fixed halving tree, the chunks added in time order: reproducible
 * bit for bit, independent of the other pixels, ~1e-16 relative per level from the
 * serial sum (sums of unit weights stay exact).  The environment variable
 * CM2_WEIGHTS_ORDER=exact keeps the serial sum for every pixel. */
int cm2_weights_accumulate(int pol, int64_t nt, int64_t npix, const int32_t *d_pix,
                           const double *d_w, const double *d_cos, const double *d_sin,
                           double *d_counts, double *d_cosine, double *d_sine,
                           double *d_cos2, double *d_sin2, double *d_sincos, void *stream);
/* cos(2 phi_t), sin(2 phi_t) for angles already resident in HBM
 * (process_ces.py:493-494; host arrays use NumPy so that they match the reference
 * bit for bit). */
int cm2_cos_sin_2phi(int64_t nt, const double *d_phi, double *d_cos, double *d_sin,
                     void *stream);
/* keep[p] = 1 for well-conditioned observed pixels: pol=1 counts>0 (:491);
 * pol>=2 |lambda_max/lambda_min| <= threshold of the QU block (:544-550);
 * pol=3 additionally counts>2 (:554-555). */
int cm2_pixel_mask(int pol, int64_t npix, const double *d_counts, const double *d_cos2,
                   const double *d_sin2, const double *d_sincos, double threshold,
                   uint8_t *d_keep, void *stream);
/* old2new[p] = rank of p among kept pixels or -1; *h_new_npix = kept count.
 * Same output as the O(Nold*Nm) search at :205-228, by prefix sum.  npix >= 1.  Synchronises. */
int cm2_pixel_compact(int64_t npix, const uint8_t *d_keep, int32_t *d_old2new,
                      int64_t *h_new_npix, void *stream);
/* d_out[old2new[p]] = d_in[p] for kept pixels (:218-219, :248-251, :280-286). */
int cm2_compact_f64(int64_t npix, const int32_t *d_old2new, const double *d_in,
                    double *d_out, void *stream);
int cm2_compact_i64(int64_t npix, const int32_t *d_old2new, const int64_t *d_in,
                    int64_t *d_out, void *stream);
/* pix[t] = old2new[pix[t]] in place, -1 stays -1 (flagging_samples :411-418). */
int cm2_flag_samples(int64_t nt, int32_t *d_pix, const int32_t *d_old2new, void *stream);

/* ------------------------------------------------------------------------- *
 * a8-a9  Per-pixel Stokes blocks
 * ------------------------------------------------------------------------- */
/* det and |det|>1e-5 mask of the per-pixel blocks, as the NumPy lines
 * linearoperators.py:792-795 (pol=3) / :820-821 (pol=2) / :789 (pol=1, counts>0). */
int cm2_bd_det_mask(int pol, int64_t npix, const double *d_counts, const double *d_cosine,
                    const double *d_sine, const double *d_cos2, const double *d_sin2,
                    const double *d_sincos, double *d_det, uint8_t *d_mask, void *stream);
/* y = M_BD x: closed-form adjugate/det per masked pixel, 0 elsewhere
 * (BlockDiagonalPreconditionerLO.mult, linearoperators.py:775-841). */
int cm2_bdprecond_apply(int pol, int64_t npix, const double *d_counts,
                        const double *d_cosine, const double *d_sine, const double *d_cos2,
                        const double *d_sin2, const double *d_sincos, const double *d_det,
                        const uint8_t *d_mask, const double *d_x, double *d_y, void *stream);
/* y = (P^T diag(N^-1) P) x per pixel (BlockDiagonalLO.mult, :728-746). */
int cm2_bd_apply(int pol, int64_t npix, const double *d_counts, const double *d_cosine,
                 const double *d_sine, const double *d_cos2, const double *d_sin2,
                 const double *d_sincos, const double *d_x, double *d_y, void *stream);

/* ------------------------------------------------------------------------- *
 * a15-a16  BLAS-1 and the PCG recurrence
 *   (utilities/linear_algebra_funcs.py:31-44; scipy.sparse.linalg.cg as called at
 *    tests/test_2level_preconditioner.py:52, src/test_BD_precond_onto_real_data.py:47)
 * ------------------------------------------------------------------------- */
/* *d_out = sum_i x_i y_i, fixed two-stage tree (bitwise reproducible run to run).
 * d_work: >= cm2_reduce_work_doubles() doubles of scratch. */
int64_t cm2_reduce_work_doubles(void);
int cm2_dot(int64_t n, const double *d_x, const double *d_y, double *d_out, double *d_work,
            void *stream);
int cm2_axpy(int64_t n, double alpha, const double *d_x, double *d_y, void *stream); /* y += alpha x */
int cm2_scal(int64_t n, double alpha, double *d_x, void *stream);
int cm2_xmy(int64_t n, const double *d_x, const double *d_y, double *d_out, void *stream); /* out = x*y */
/* p = z + (rho/rho_prev) p   with rho, rho_prev read from device memory
 * (cg: beta = rho_cur/rho_prev; p *= beta; p += z). */
int cm2_pcg_update_p(int64_t n, const double *d_rho, const double *d_rho_prev,
                     const double *d_z, double *d_p, void *stream);
/* alpha = rho/pq (device scalars); x += alpha p; r -= alpha q; *d_rr = r.r */
int cm2_pcg_update_xr(int64_t n, const double *d_rho, const double *d_pq, const double *d_p,
                      const double *d_q, double *d_x, double *d_r, double *d_rr,
                      double *d_work, void *stream);

/* The whole solve for hosts that are not Python: scipy.sparse.linalg.cg's recurrence (the driver the
 * reference calls: tests/test_2level_preconditioner.py:52, src/test_BD_precond_onto_real_data.py:47)
 * with the operator A and the preconditioner M (may be NULL) as callbacks on device vectors.
 * A callback computes d_out = Op d_in on `stream` and returns 0 on success.  x_is_zero != 0: d_x is
 * overwritten with the start vector 0, otherwise d_x holds x0.  Stops when ||r||_2 < max(atol,
 * rtol ||b||_2), tested before each iteration like scipy does; maxiter < 0 means 10 n.
 * *h_iters = iterations done, *h_info = 0 (converged) or maxiter.  `callback` (may be NULL) is
 * called after every iteration with the iteration number, the iterate (device) and ||r||_2. */
typedef int (*cm2_apply_fn)(void *ctx, const double *d_in, double *d_out, void *stream);
typedef void (*cm2_iter_fn)(void *ctx, int64_t iteration, const double *d_x, double rnorm);
int cm2_pcg(int64_t n, cm2_apply_fn A, void *A_ctx, cm2_apply_fn M, void *M_ctx,
            const double *d_b, double *d_x, int x_is_zero, double rtol, double atol,
            int64_t maxiter, cm2_iter_fn callback, void *cb_ctx, int64_t *h_iters, int *h_info,
            void *stream);

/* (e) The same solve on TOD shards, one process per GPU (the reference is one process: its
 * block independence, interfaces/blkop.py:195-206, is what makes the cut exact).  The library links no
 * collective library: the HOST passes its own reduction -- `reduce` combines `count` doubles at d_vals
 * over all ranks IN PLACE, queued on `stream`, CM2_REDUCE_SUM or CM2_REDUCE_MAX (INTEGRATION.md shows
 * the three-line RCCL form) -- and does the map-sized exchange inside its operator callback.
 *   CM2_LAYOUT_REPLICATED: every rank holds whole map vectors (n_local = n); the A callback applies the
 *     rank's P^T N^-1 P and all-reduces the product; dots are computed redundantly, b.b and ||r||^2 are
 *     MAX-reduced so that every rank takes the same stop decision.
 *   CM2_LAYOUT_ROWS: every vector (d_b, d_x, the callbacks' arguments) is the rank's n_local rows; the A
 *     callback all-gathers its input and reduce-scatters the product; b.b, rho, p.q and ||r||^2 are
 *     SUM-reduced (three 8-byte reductions an iteration); maxiter < 0 means 10 x the summed n_local.
 * Every rank must make the call with the same rtol / atol / maxiter; they return the same *h_iters and
 * *h_info.  Same recurrence and stop rule as cm2_pcg. */
#define CM2_REDUCE_SUM 0
#define CM2_REDUCE_MAX 1
#define CM2_LAYOUT_REPLICATED 0
#define CM2_LAYOUT_ROWS 1
typedef int (*cm2_reduce_fn)(void *ctx, double *d_vals, int64_t count, int op, void *stream);
int cm2_pcg_sharded(int64_t n_local, cm2_apply_fn A, void *A_ctx, cm2_apply_fn M, void *M_ctx,
                    const double *d_b, double *d_x, int x_is_zero, double rtol, double atol,
                    int64_t maxiter, cm2_iter_fn callback, void *cb_ctx, int layout,
                    cm2_reduce_fn reduce, void *reduce_ctx, int64_t *h_iters, int *h_info,
                    void *stream);

/* a13  arnoldi (interfaces/deflationlib.py:17-113) as a C entry point, operator as a callback:
 * modified Gram-Schmidt on r0 = b - A x0 (d_x0 may be NULL = 0) with the reference's early exit
 * (||r0|| < tol ||b|| or < tol: *h_steps = 0, :80-82), its stop rule |v_new[j] h_{j+1,j}| <= tol
 * (:101) and its failure after inner_m steps (returns non-zero, cm2_last_error() =
 * "Convergence not achieved within the Arnoldi algorithm", :111-112; *h_steps = inner_m).
 * d_V: inner_m vectors of n doubles, vector i at d_V + i*n; h_H: (inner_m + 1) x inner_m,
 * row-major, host; on return the first *h_steps vectors and columns are set (build_hess :115-137
 * reads its m x m matrix from the leading block). */
int cm2_arnoldi(int64_t n, cm2_apply_fn A, void *A_ctx, const double *d_b, const double *d_x0,
                double tol, int inner_m, double *d_V, double *h_H, int *h_steps, void *stream);

/* ------------------------------------------------------------------------- *
 * a10-a12  Deflation space and coarse operator
 *   (DeflationLO linearoperators.py:1029-1065, CoarseLO :946-1027,
 *    M2 src/test_M2_precond_onto_real_data.py:98-112)
 *   Z is n x r, ROW-major in HBM (the r entries of one map element contiguous).
 * ------------------------------------------------------------------------- */
int cm2_Zt_apply(int64_t n, int r, const double *d_Z, const double *d_x, double *d_out,
                 double *d_work, void *stream);                 /* out[r] = Z^T x  (:1051-1056) */
int cm2_Z_apply(int64_t n, int r, const double *d_Z, const double *d_y, double *d_out,
                void *stream);

/* w += alpha * Z y for a row-major n x r panel Z: the update step of the Arnoldi
 * orthogonalisation (w -= V h, interfaces/deflationlib.py:88-93 -- the reference's loop of r
 * axpy calls) in one pass over the panel; the order of the r terms is a fixed tree, not the
 * k = 0..r-1 order of cm2_Z_apply. */
int cm2_Z_axpy(int64_t n, int r, const double *d_Z, const double *d_y, double alpha,
               double *d_w, void *stream);                                  /* out[n] = Z y    (:1041-1050) */
/* E[r1 x r2] (row-major) = Z1^T Z2, fp64 MFMA panels when r1,r2 are multiples of
 * 16 (CoarseLO.__init__: dgemm(Z, Az.T), :1019).  d_work >= cm2_gemm_tn_work_doubles(r1,r2). */
int64_t cm2_gemm_tn_work_doubles(int r1, int r2);
int cm2_gemm_tn(int64_t n, int r1, int r2, const double *d_Z1, const double *d_Z2, double *d_E,
                double *d_work, void *stream);
/* C[m x n] (row-major) = A^T B^T with A k x m and B n x k, both row-major: the
 * reference's dgemm(A,B) helper (utilities/linear_algebra_funcs.py:16-29). */
int cm2_gemm_atbt(int64_t m, int64_t n, int64_t k, const double *d_A, const double *d_B,
                  double *d_C, void *stream);
/* d_out[c][r] = d_in[r][c] for a row-major rows x cols matrix: layout change between a set of
 * contiguous map vectors (cols x n) and the row-major n x r panel that DeflationLO streams
 * (the reference keeps Z as a list of column views, linearoperators.py:1059-1062). */
int cm2_transpose(int64_t rows, int64_t cols, const double *d_in, double *d_out, void *stream);
/* d_out[n x rout] (+)= d_P[n x rin] d_W[rin x rout], all row-major, accumulate != 0 adds to d_out:
 * the tall-panel products of the deflation build -- Ritz vectors Z = V y (build_Z,
 * deflationlib.py:183) and A Z = P_{m+1} (H y) through the Arnoldi relation instead of r more
 * applications of A (src/test_M2_precond_onto_real_data.py:98-101); fp64 MFMA for rin = 32,
 * rout = 16 / 32. */
int cm2_panel_gemm(int64_t n, int rin, int rout, const double *d_P, const double *d_W,
                   double *d_out, int accumulate, void *stream);
/* out[r] = M[r x r] (row-major) v  -- E^-1 held as an explicit small matrix */
int cm2_small_matvec(int r, const double *d_M, const double *d_v, double *d_out, void *stream);
/* fused second half of M2 r = M_BD (r - AZ y) + Z y  given y = E^-1 Z^T r:
 * one pass over Z and AZ, then the per-pixel M_BD block. */
int cm2_m2_finish(int pol, int64_t npix, int r, const double *d_Z, const double *d_AZ,
                  const double *d_y, const double *d_res, const double *d_counts,
                  const double *d_cosine, const double *d_sine, const double *d_cos2,
                  const double *d_sin2, const double *d_sincos, const double *d_det,
                  const uint8_t *d_mask, double *d_out, void *stream);

/* ---- f1: sub-scan filtering of a time stream --------------------------------
 * Replaces FilterLO (interfaces/linearoperators.py:94-322).  The time stream is
 * cut into `nseg` chunks (one per CES x detector pair x sub-scan, the loops at
 * :134-140); h_start must be ascending and the chunks must not overlap.
 * Samples outside every chunk are 0 in the output (vec_out = d*0, :130).
 * Flags (pixel id < 0) are read from d_pix at create time and at every apply;
 * they must not change in between (the per-chunk bases below depend on them).
 *
 * order == 0  (FilterLO.mult :129-168): out = d - mean(unflagged d) on every
 *   sample of the chunk; a chunk without unflagged samples (or with a non-finite
 *   mean) stays 0.  h_table_off/h_table are ignored (may be NULL).
 * order  > 0  (globalprocsfilter :286-322): K = order+1 (K <= 8).  h_table holds
 *   one n x K row-major block of normalised Legendre columns for every distinct
 *   chunk length n (get_legendre_polynomials, utilities/linear_algebra_funcs.py:
 *   47-59); h_table_off[s] is the offset (in doubles) of chunk s's block.  Per chunk,
 *   with m the number of unflagged samples:
 *     m <= order : chunk left at 0 (:303-304);
 *     m == n     : out = d - sum_k <L_k,d> L_k with the table columns as they are
 *                  (:317-321);
 *     otherwise  : out = d - Q Q^T d on the unflagged samples and 0 on the flagged
 *                  ones, Q an orthonormal basis of the polynomials of degree <= order
 *                  on the unflagged samples (:307-315, where Q comes from
 *                  qr(legendres[unflagged])).  Here Q is built once at create time
 *                  from the three-term recurrence of the discrete orthogonal
 *                  polynomials of those samples; same projector, and no loss of
 *                  orthogonality when the restricted Legendre block is ill
 *                  conditioned. */
typedef struct cm2_filter cm2_filter;
int cm2_filter_create(cm2_filter **out, int64_t nt, int64_t nseg, const int64_t *h_start,
                      const int64_t *h_len, const int32_t *d_pix, int order,
                      const int64_t *h_table_off, const double *h_table, int64_t table_len,
                      void *stream);
void cm2_filter_destroy(cm2_filter *f);
/* info[7] = nt, nseg, order, samples inside chunks, then (order > 0) the number of
 * chunks skipped / without flags / with flags */
int cm2_filter_info(const cm2_filter *f, int64_t *info);
/* d_out = F d_in (nt doubles each; d_out must not alias d_in) */
int cm2_filter_apply(const cm2_filter *f, const double *d_in, double *d_out, void *stream);

/* The same filter with input and output in the tile-bucketed order of `tiles` (flagged samples
 * have no slot there).  The time stream is cut into windows of <= 8192 samples holding whole
 * chunks; each window is gathered through an address-sorted list, filtered in LDS and
 * scattered back.  *h_done = 0 (and nothing is written) when a chunk is longer than a window:
 * the caller then applies cm2_filter_apply on the time order.  d_out_tb != d_in_tb. */
int cm2_filter_apply_tiles(cm2_filter *f, const cm2_tiles *tiles, const double *d_in_tb,
                           double *d_out_tb, int *h_done, void *stream);

/* ---- f2: ground-template filter  (GroundFilterLO, :24-61) --------------------
 * d_out[t] = d_v[t] - binned[d_bin[t]]   (d_out[t] = d_v[t] where d_bin[t] < 0),
 * the last step of v - G (G^T G)^-1 G^T v once binned = (G^T G)^-1 G^T v has
 * been formed with cm2_Pt_apply and cm2_bdprecond_apply (pol = 1). */
/* d_sums[b] = sum of d_v[t] over the samples with d_bin[t] == b  (G^T v, pol = 1) for
 * nbins <= 8192: LDS histogram per workgroup, then atomic adds -- the order of the terms
 * is not fixed (equal to the serial loop :394-400 to rounding).  More bins: cm2_Pt_apply. */
int cm2_ground_bin_sums(int64_t nt, int nbins, const int32_t *d_bin, const double *d_v,
                        double *d_sums, void *stream);
int cm2_ground_subtract(int64_t nt, const int32_t *d_bin, const double *d_binned,
                        const double *d_v, double *d_out, void *stream);

/* ---- f2b: the same bin sums, bitwise reproducible  (GroundFilterLO(..., reproducible=True)) ----
 * d_sums[b] = sum of d_v[t] over the samples with d_bin[t] == b, in place of the serial loop of the reference
 * (linearoperators.py:394-400), as an ORDER-INDEPENDENT sum: the same bits run to run, for the time order and the
 * tile order, for every permutation of the samples and every launch shape.  A sample counts when
 * 0 <= d_bin[t] < nbins; every other label is skipped, as cm2_ground_bin_sums does.
 *   1. Scale.  M = max over the counted samples of the bit pattern of |v_t| read as a uint64 (monotonic for
 *      non-negative doubles; Inf and NaN sort above every finite value): one pass, one 64-bit atomic max on a
 *      device word, exact and independent of the order.
 *        M == 0, or no counted sample:        every sum is +0.0.
 *        M >= 0x7FF0000000000000 (a counted sample is Inf or NaN): EVERY sum is NaN.  cm2_ground_bin_sums poisons
 *                                             only the bins such a sample falls into; this route poisons them all.
 *        otherwise e = (M >> 52) - 1023, so that every counted |v_t| < 2^(e+1).
 *   2. Limbs.  Per counted sample, all in fp64 and all exact (scalings by powers of two with ldexp, subtractions
 *      of a truncation):
 *        y0 = ldexp(v, 31 - e), l0 = trunc(y0), r = y0 - l0;  y1 = ldexp(r, 32), l1 = trunc(y1), r = y1 - l1;
 *        l2 = trunc(ldexp(r, 32)).
 *      Each |l_k| < 2^32, all three carry the sign of v, and l0 2^64 + l1 2^32 + l2 = trunc(v 2^(95-e)).  Each
 *      non-zero limb, converted to int64, is added to its bin's accumulator L_k with an unsigned 64-bit integer
 *      atomic add (two's complement makes it signed).  Integer adds are exact: any order gives the same L_k.
 *      nt < 2^31 keeps every |L_k| below 2^63.  The translation unit is compiled without FMA contraction.
 *   3. Finish.  One thread per bin: S = L0 2^64 + L1 2^32 + L2 (|S| < 2^127) in 128-bit integers; of |S| the top
 *      53 bits are kept, rounded to nearest, ties to even, on the rest; sum = +-ldexp(mant, shift + e - 95).
 * So d_sums[b] is the correctly rounded sum of the truncated terms trunc(v_t 2^(95-e)) 2^(e-95).  Against the real
 * sum it is off by at most half an ulp of the result plus hits_b 2^(e-95).  The bits are pinned for
 * 2^-900 <= max |v_t| <= 2^900; outside, the recipe still defines the value, but the result may be subnormal or
 * overflow and its last bit is not part of the contract.
 *
 * cm2_ground_sums_create: the handle owns 3 nbins int64 limbs and the scale word.  Allocates.
 * cm2_ground_sums_info: h_info[4] = nbins, the bin limit of the LDS route (2048), the dynamic LDS bytes of the LDS
 *   route at nbins (3 x 8 x nbins; 0 above the limit), the route that route = 0 takes (1 or 2).
 * cm2_ground_sums_apply: overwrites d_sums[nbins].  route 1: three limb histograms per workgroup in LDS, then
 *   integer atomics of the non-zero entries to the global limbs (nbins <= 2048); route 2: integer atomics straight to
 *   the global limbs (any nbins); route 0: 1 where it fits, else 2.  Both routes give the same bits.  Clears its
 *   state with a memset on the stream, then launches kernels only: it allocates nothing and does not synchronise.
 *   One handle runs one apply at a time.
 * Refused with CM2_ERR_ARGUMENT before any HIP call: NULL pointers (d_bin and d_v may be NULL when nt == 0),
 * nbins < 1, nt < 0, nt >= 2^31, a route outside 0..2, route 1 with nbins > 2048. */
typedef struct cm2_ground_sums cm2_ground_sums;
int cm2_ground_sums_create(cm2_ground_sums **out, int nbins, void *stream);
int cm2_ground_sums_destroy(cm2_ground_sums *h);
int cm2_ground_sums_info(const cm2_ground_sums *h, int64_t *h_info);
int cm2_ground_sums_apply(cm2_ground_sums *h, int64_t nt, const int32_t *d_bin, const double *d_v, int route,
                          double *d_sums, void *stream);

/* ---- f2c: HWP-synchronous signal filter  (HWPSSFilterLO) ------------------------------------
 * Fits and removes the harmonics of the half-wave plate angle, per detector and chunk.  No counterpart in the
 * reference: the definition is the one below.
 * Layout as cm2_pointing_expand writes it: nt = ndet ns, sample t of detector k at k ns + t.  d_chi[ns] is the plate
 * angle in radians, shared by all detectors; a sample is flagged where d_pix[nt] < 0.  The chunk edges
 * 0 = e_0 < e_1 < ... < e_C = ns cut the time axis, the same for every detector; a unit is one (detector, chunk) pair,
 * unit k C + c.  Templates for H = nharm harmonics, 1 <= H <= CM2_HWPSS_MAX_HARM, K = 2 H + 1:
 *     T_0 = 1,  T_{2n-1}(t) = cos(n chi_t),  T_{2n}(t) = sin(n chi_t)   (n = 1..H).
 * Per unit, V its unflagged samples and m = |V|:
 *     G = sum_{t in V} T(t) T(t)^T,   b = sum_{t in V} T(t) v_t,   c = G^-1 b,
 *     out_t = v_t - T(t)^T c on V,  out_t = 0 on the flagged samples of the unit
 * (M - M T G^-1 T^T M with M the mask: symmetric and idempotent).
 * A unit is SKIPPED -- every sample of it 0 in the output, its K coefficients 0 -- when
 *     m < K, or
 *     the Cholesky factorisation G = L L^T meets a pivot p_j = G_jj - sum_{k<j} L_jk^2 <= CM2_HWPSS_TAU G_jj
 *     (it stops at the first such pivot): the plate covered too little angle in the chunk, the harmonics are
 *     collinear there and a fit would amplify rounding by 1 / pivot.
 * A non-finite v_t on an unflagged sample makes its own unit's output non-finite and no other unit's.
 *
 * G depends on chi and the flags only: it is formed and factorised on the device by cm2_hwpss_create.  The handle
 * holds the factors (K (K + 1) / 2 doubles per unit), the skip marks, the tables cos chi and sin chi (ns doubles
 * each, device sincos, once) and the segment sums of one application (K doubles per segment).  The harmonics
 * n >= 2 come from the two tables by c_n = c_{n-1} c_1 - s_{n-1} s_1, s_n = s_{n-1} c_1 + c_{n-1} s_1 in registers;
 * nothing of size nt K is ever stored.
 *
 * Order of the sums (no floating-point atomics; the same bits every time): a unit is cut into segments of 4096
 * samples (the last one shorter), one workgroup of 256 threads each.  Thread t adds T_j(q) v_q over its unflagged
 * samples q = t, t + 256, ... of the segment in ascending order, starting from 0; the 64 lanes of a wave are added
 * by x += x[lane + off], off = 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3; a unit's segments in
 * ascending order, starting from 0.  The Gram sums are formed the same way.  Then the two triangular solves (row i:
 * the known terms subtracted in ascending index order, then the division by L_ii), and
 * out_t = v_t - (((c_0 + c_1 T_1) + c_2 T_2) + ... + c_{K-1} T_{K-1}).  Every product and sum is rounded on its own.
 *
 * cm2_hwpss_create keeps d_pix (it must not change or be freed while the handle lives) and copies what it needs of
 *   d_chi.  h_edges[nchunks + 1].  Allocates and synchronises.
 * cm2_hwpss_info: h_info[9] = ns, ndet, nchunks, nharm, units fitted, units skipped for m < K, units skipped for a
 *   pivot, segment size, segments.
 * cm2_hwpss_apply: d_out = F d_in (nt doubles each).  Three launches, no allocation, no synchronisation.  One handle
 *   runs one apply or fit at a time.
 * cm2_hwpss_fit: d_coeff[ndet nchunks K] = the coefficients c of every unit, without the subtract pass.
 * cm2_hwpss_tables: copies the two tables to d_cos[ns], d_sin[ns].
 * Refused with CM2_ERR_ARGUMENT, the outputs (and *out) untouched: nharm outside [1, 8]; ns, ndet or nchunks < 1;
 * edges that do not ascend strictly from 0 to ns; NULL pointers; sizes that overflow the index types (ns >= 2^40,
 * ndet ns > 2^46, 2^31 or more segments or units); d_out or d_coeff sharing memory with d_in. */
#define CM2_HWPSS_TAU 0.0009765625          /* 2^-10 */
#define CM2_HWPSS_MAX_HARM 8
typedef struct cm2_hwpss cm2_hwpss;
int cm2_hwpss_create(cm2_hwpss **out, int64_t ns, int ndet, int64_t nchunks, const int64_t *h_edges,
                     const double *d_chi, const int32_t *d_pix, int nharm, void *stream);
int cm2_hwpss_destroy(cm2_hwpss *h);
int cm2_hwpss_info(const cm2_hwpss *h, int64_t *h_info);
int cm2_hwpss_apply(cm2_hwpss *h, const double *d_in, double *d_out, void *stream);
int cm2_hwpss_fit(cm2_hwpss *h, const double *d_in, double *d_coeff, void *stream);
int cm2_hwpss_tables(const cm2_hwpss *h, double *d_cos, double *d_sin, void *stream);

/* ---- f2d: common-mode filter  (CommonModeFilterLO) ------------------------------------------
 * Fits and removes focal-plane modes across the detectors, per group of detectors and time sample: the common mode
 * of a wafer, its gradient and curvature over the focal plane.  No counterpart in the reference: the definition is
 * the one below.
 * Layout as cm2_pointing_expand writes it: nt = ndet ns, sample i of detector k at k ns + i, flagged where
 * d_pix[nt] < 0.  The group edges 0 = g_0 < g_1 < ... < g_G = ndet cut the detectors into G contiguous groups (wafers,
 * frequency bands).  Every detector carries K template values Phi[k, 0..K-1], 1 <= K <= CM2_CMODE_MAX_K,
 * d_modes[k K + j]; they do not depend on time.  A unit is one (group, time sample) pair, unit g ns + i.
 * Per unit, V the unflagged detectors of the group at sample i and m = |V|:
 *     G = sum_{k in V} Phi_k Phi_k^T,   b = sum_{k in V} Phi_k v[k, i],   c = G^-1 b,
 *     out[k, i] = v[k, i] - Phi_k^T c on V,  out[k, i] = 0 on the flagged samples of the unit
 * (M - M Phi G^-1 Phi^T M with M the mask: symmetric, idempotent, and it annihilates Phi c for any c).
 * K = 1 with Phi = 1 is the plain common mode, K = 1 with Phi = the relative gains the gain-weighted one;
 * K = 3, 6, 10 are the monomials of total degree <= 1, 2, 3 in the focal-plane coordinates.
 * A unit is SKIPPED -- every sample of it 0 in the output, its K coefficients 0 -- when
 *     m < K, or
 *     the Cholesky factorisation G = L L^T meets a pivot p_j = G_jj - sum_{k<j} L_jk^2 <= CM2_CMODE_TAU G_jj
 *     (it stops at the first such pivot): the surviving detectors do not span the templates.
 * Every unit has a class: CM2_CMODE_FITTED, CM2_CMODE_EMPTY (m = 0), CM2_CMODE_FEW (0 < m < K), CM2_CMODE_PIVOT.
 * The class depends on Phi and the flags only.  A non-finite v[k, i] on an unflagged sample makes its own unit's
 * output non-finite and no other unit's.
 *
 * The handle holds Phi (ndet K doubles), the group edges and one class byte per unit.  G is formed from the flags in
 * registers on every call; nothing of size ns K^2 is stored.
 *
 * Order (no floating-point atomics, no sums across threads; the same bits every time): one thread per unit.  G_ab
 * (a >= b) and b_a start at 0 and take G_ab += Phi_ka Phi_kb, b_a += Phi_ka v[k, i] over the unflagged detectors of
 * the group in ascending k.  The factor is formed row by row, p_j = G_jj - L_j0^2 - ... - L_j,j-1^2 (left to right),
 * L_jj = sqrt(p_j), L_ij = (G_ij - L_i0 L_j0 - ... - L_i,j-1 L_j,j-1) / L_jj; then the two triangular solves (row i:
 * the known terms subtracted in ascending index order, then the division by L_ii), and
 * out[k, i] = v[k, i] - (((c_0 Phi_k0 + c_1 Phi_k1) + c_2 Phi_k2) + ... + c_{K-1} Phi_k,K-1).  Every product and sum is
 * rounded on its own.  The result of a unit does not depend on ns, on the other groups or on where the unit lies.
 *
 * cm2_cmode_create keeps d_pix (it must not change or be freed while the handle lives) and copies d_modes[ndet K]
 *   and h_group_edges[ngroups + 1]; classes every unit and counts the classes.  Allocates and synchronises.
 * cm2_cmode_info: h_info[8] = ns, ndet, ngroups, K, units fitted, empty, few, pivot.
 * cm2_cmode_apply: d_out = F d_in (nt doubles each).  One launch, no allocation, no synchronisation.  d_out may be
 *   d_in itself (a thread reads its column before it stores and touches no other); any other overlap is refused.
 * cm2_cmode_fit: d_coeff[(g K + j) ns + i] = c_j of unit (g, i), 0 for a skipped unit; nothing is subtracted.
 * cm2_cmode_status: d_status[g ns + i] = the class of unit (g, i), one byte each.  Synchronises.
 * Refused with CM2_ERR_ARGUMENT, the outputs (and *out) untouched: K outside [1, 10]; ns, ndet or ngroups < 1; edges
 * that do not ascend strictly from 0 to ndet; NULL pointers; sizes that overflow the index types or the grid
 * (ndet ns > 2^46, ndet >= 2^31, 2^31 or more workgroups of 256 units); d_out overlapping d_in without being d_in;
 * d_coeff sharing memory with d_in. */
#define CM2_CMODE_TAU 0.0009765625          /* 2^-10 */
#define CM2_CMODE_MAX_K 10
#define CM2_CMODE_FITTED 0
#define CM2_CMODE_EMPTY 1
#define CM2_CMODE_FEW 2
#define CM2_CMODE_PIVOT 3
typedef struct cm2_cmode cm2_cmode;
int cm2_cmode_create(cm2_cmode **out, int64_t ns, int ndet, int ngroups, const int64_t *h_group_edges, int K,
                     const double *d_modes, const int32_t *d_pix, void *stream);
int cm2_cmode_destroy(cm2_cmode *h);
int cm2_cmode_info(const cm2_cmode *h, int64_t *h_info);
int cm2_cmode_apply(cm2_cmode *h, const double *d_in, double *d_out, void *stream);
int cm2_cmode_fit(cm2_cmode *h, const double *d_in, double *d_coeff, void *stream);
int cm2_cmode_status(const cm2_cmode *h, uint8_t *d_status);

/* ---- f2e: glitch flags  (GlitchFlagger, flag_glitches, apply_flags) ----------------------------
 * Flags cosmic-ray hits, short readout jumps and non-finite samples of a time stream from the data: per noise block
 * a running median is subtracted, the median absolute deviation of the residual gives a robust scale, samples beyond
 * nsigma scales are hits and every hit grows by a few samples.  No counterpart in the reference: the definition is
 * the one below.  Every result is an order statistic, a comparison or an integer count, so it does not depend on how
 * it is computed: the same bits every time, on every layout of threads.
 * Inputs: d[nt]; noise blocks of sizes[0..nblocks-1] samples adding up to nt (BlockLO's convention); optional flags
 * in the two encodings of cm2_gaps_create (flag_kind 0: int32, flagged when negative; 1: bytes, flagged when
 * non-zero; d_flags NULL: nothing flagged); the half-width 1 <= h <= CM2_GLITCH_MAX_HALF_WIDTH, W = 2 h + 1; nsigma
 * finite and > 0; 0 <= grow <= CM2_GLITCH_MAX_GROW; optionally prev[nt], the class bytes of an earlier pass.
 * All windows and neighbourhoods are cut at the block boundaries.
 *  1. usable_i: the sample is not flagged, d_i is finite and prev_i (if given) is neither HIT nor NEAR.
 *  2. For a usable i the window is the usable j of the same block with |j - i| <= h: m_i >= 1 values, ascending
 *     v_0 <= ... <= v_{m-1}.  m odd: med_i = v_{(m-1)/2}; m even: med_i = 0.5 v_{m/2-1} + 0.5 v_{m/2} (two exact
 *     halvings and one addition: no overflow).
 *  3. r_i = d_i - med_i for a usable i, r_i = 0 otherwise.
 *  4. m_b = the usable samples of block b.  m_b < W: the block is short and sigma_b = +inf.  Otherwise s_b is the
 *     order statistic of rank (m_b - 1) / 2 (0-based, the lower median) of |r_i| over the usable samples of the block
 *     and sigma_b = CM2_GLITCH_MAD_TO_SIGMA s_b, one multiplication.  A sigma given by the caller replaces it.
 *  5. thr_b = nsigma sigma_b, one multiplication; hit_i: usable_i and |r_i| > thr_b (equality is no hit; sigma_b = 0
 *     makes every non-zero residual a hit, sigma_b = +inf none).
 *  6. The class of a sample, the first rule that applies: CM2_GLITCH_INPUT flagged on input; CM2_GLITCH_NONFINITE
 *     d_i not finite; prev_i where that is HIT or NEAR; CM2_GLITCH_HIT hit_i; CM2_GLITCH_NEAR some hit j != i of the
 *     same block with |j - i| <= grow; CM2_GLITCH_CLEAN.
 *  7. counts[b][c], int64: the samples of class c in block b.
 * Iterating (glitches bias the medians and inflate the scale) is the caller's loop: pass k runs 1-7 with prev = the
 * classes of pass k - 1.  Which of -0.0 and +0.0 a median returns is not specified; it can change the sign of a
 * zero residual only.
 *
 * cm2_glitch_create copies h_sizes; the handle owns the block tables, the per-block histograms of the selection
 *   (nblocks x 2048 x 4 bytes) and its per-block state, and no nt-sized buffer.  Allocates and synchronises.
 * cm2_glitch_info: h_info[6] = nt, nblocks, h, outputs per thread of the median kernel, tier of h (0-3: the window in
 *   registers, h <= 8 / 16 / 32 / 48; 4: 96 keys in registers, the rest in LDS), bytes owned.
 * cm2_glitch_residual: d_r = r (definitions 1-3).  One launch.
 * cm2_glitch_scale: d_sigma[nblocks] = sigma (definition 4) from d_r as cm2_glitch_residual made it with the same
 *   flags and prev.  Six passes over d_r and the flags (d_in is read only where r = 0), no sort.  Uses the handle's
 *   histograms: one call at a time per handle.
 * cm2_glitch_classify: d_class[nt] (one byte each) and d_counts[nblocks][5] (definitions 5-7).  d_class must not be
 *   d_prev: a workgroup reads prev in the halo of its tile, where another one writes.
 * cm2_glitch_apply_pix: d_pix[i] = -1 where d_class[i] != 0, in place.
 * The stream-sized calls allocate nothing and do not synchronise.  Refused with CM2_ERR_ARGUMENT, the outputs (and
 * *out) untouched: h outside [1, 64]; nt < 1 or nt >= 2^32 - 1 (the limit of cm2_gaps); sizes that are not positive
 * or do not add up to nt; more than 2^18 blocks; NULL pointers (d_flags and d_prev may be NULL); a flag_kind other
 * than 0 or 1 with flags given; nsigma not finite or <= 0; grow outside [0, 64]; an output that overlaps an input or
 * another output. */
#define CM2_GLITCH_MAD_TO_SIGMA 1.4826
#define CM2_GLITCH_MAX_HALF_WIDTH 64
#define CM2_GLITCH_MAX_GROW 64
#define CM2_GLITCH_CLEAN 0
#define CM2_GLITCH_INPUT 1
#define CM2_GLITCH_NONFINITE 2
#define CM2_GLITCH_HIT 3
#define CM2_GLITCH_NEAR 4
typedef struct cm2_glitch cm2_glitch;
int cm2_glitch_create(cm2_glitch **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, int half_width,
                      void *stream);
int cm2_glitch_destroy(cm2_glitch *h);
int cm2_glitch_info(const cm2_glitch *h, int64_t *h_info);
int cm2_glitch_residual(cm2_glitch *h, const double *d_in, const void *d_flags, int flag_kind, const uint8_t *d_prev,
                        double *d_r, void *stream);
int cm2_glitch_scale(cm2_glitch *h, const double *d_in, const double *d_r, const void *d_flags, int flag_kind,
                     const uint8_t *d_prev, double *d_sigma, void *stream);
int cm2_glitch_classify(cm2_glitch *h, const double *d_in, const double *d_r, const void *d_flags, int flag_kind,
                        const uint8_t *d_prev, const double *d_sigma, double nsigma, int grow, uint8_t *d_class,
                        int64_t *d_counts, void *stream);
int cm2_glitch_apply_pix(int64_t nt, const uint8_t *d_class, int32_t *d_pix, void *stream);

/* ---- f2f: baseline jumps  (JumpCorrector, correct_jumps) ----------------------------------------
 * Finds the steps in the level of a time stream (flux jumps of the readout, relocks), estimates their heights,
 * subtracts the accumulated offsets and classes the samples around each step, per noise block.  The glitch flagger
 * cannot see a step: a running median keeps an edge.  No counterpart in the reference: the definition is the one
 * below, and every result has the bits it gives, on every run and every layout of threads.
 * Inputs: d[nt]; noise blocks of sizes[0..nblocks-1] samples adding up to nt (BlockLO's convention), block b the
 * samples [start_b, end_b); optional flags in the two encodings of cm2_gaps_create (flag_kind 0: int32, flagged when
 * negative; 1: bytes, flagged when non-zero; d_flags NULL: nothing flagged); optionally prev[nt], class bytes of the
 * glitch flagger or of an earlier pass, non-zero meaning unusable; the half-window 1 <= w <= CM2_JUMP_MAX_WINDOW;
 * 1 <= min_count <= w; nsigma finite and > 0; 0 <= radius <= CM2_JUMP_MAX_RADIUS.  Everything is cut at the block
 * boundaries.  Every operation on doubles named below is rounded once (no fused multiply-add).
 *  1. usable_j: the sample is not flagged, d_j is finite and prev_j == 0 (or prev is NULL).
 *  2. Window sum, for j with start_b <= j and j + w <= end_b: S_j = the sum of the usable d_k, k = j .. j + w - 1, in
 *     ascending k, starting from +0.0; n_j = the number of usable samples among them.  (Adding +0.0 for an unusable
 *     sample gives the same bits as skipping it.)
 *  3. Step statistic, for i with start_b + w <= i <= end_b - w: L = S_{i-w}, nL = n_{i-w}, R = S_i, nR = n_i.
 *     evaluable_i: nL >= min_count, nR >= min_count and t_i = R / nR - L / nL is finite (two divisions, one
 *     subtraction).  Wherever a position is not evaluable -- every position within w of a block end, every block
 *     shorter than 2 w -- t_i = +0.0 and noeval_i = 1.
 *  4. Scale: e_b = the evaluable positions of block b.  e_b < 3: the block is short and sigma_b = +inf.  Otherwise
 *     sigma_b = CM2_GLITCH_MAD_TO_SIGMA x the order statistic of rank (e_b - 1) / 2 (0-based) of |t_i| over the
 *     evaluable positions: definition 4 of f2e with d = r = t, the noeval bytes as flags and h = 1.  A sigma given by
 *     the caller replaces it; it is the scale of t, not of d.
 *  5. Candidate: evaluable_i and |t_i| > nsigma sigma_b (one multiplication; equality is no candidate).
 *  6. Jump: a candidate p with no evaluable j of the block, 0 < |j - p| <= w, such that |t_j| > |t_p|, or
 *     |t_j| == |t_p| and j < p.  Its height is a_p = t_p.
 *  7. The jump table: the positions of the jumps ascending (index into the stream, int64), their heights, and
 *     njumps_b per block.  With more jumps than the caller's capacity the true counts are still reported and nothing
 *     beyond the capacity is written.
 *  8. Correction: block b has the jumps p_1 < ... < p_k; s_0 = +0.0, s_m = s_{m-1} + a_{p_m}; d_out_i = d_i - s_{m(i)}
 *     with m(i) = #{p <= i}, for every sample, flagged ones included (a non-finite d_i stays non-finite).
 *  9. The class of a sample, the first rule that applies: (a) prev_i if non-zero; (b) CM2_JUMP_AT where i is a jump;
 *     (c) CM2_JUMP_NEAR where some jump p != i of the block has |i - p| <= radius; (d) CM2_JUMP_CLEAN.
 *     counts[b][3], int64: the samples of block b that rules b-d gave CLEAN, AT, NEAR (those with prev_i are in none).
 * Iterating is the caller's loop: a jump within w of a larger one is suppressed by rule 6 and shows once the larger one
 * is removed.  Pass k runs 1-9 on the output of pass k - 1 with the classes of pass k - 1 as prev.
 *
 * cm2_jump_create copies h_sizes; the handle owns the block tables, one mark byte per sample, the temporary storage
 *   of the select that makes the table, and a cm2_glitch of half-width 1 for the scale.  Allocates and synchronises.
 * cm2_jump_info: h_info[6] = nt, nblocks, w, positions per workgroup, LDS bytes of a workgroup of the statistic kernel,
 *   bytes owned.
 * cm2_jump_stat: d_t[nt] and d_noeval[nt] (one byte each), rules 1-3.  One launch.
 * cm2_jump_scale: d_sigma[nblocks], rule 4, by cm2_glitch_scale: one call at a time per handle.
 * cm2_jump_find: rules 5-7 and the chain of rule 8.  d_njumps[nblocks + 1] = njumps_b and, last, their sum;
 *   d_pos[capacity], d_heights[capacity] and d_offsets[capacity] = p, a_p and s_m of the first min(sum, capacity)
 *   jumps, the rest untouched.  Uses the handle's mark bytes: one call at a time per handle.
 * cm2_jump_correct: d_out[nt], d_class[nt] and d_counts[nblocks][3] (rules 8 and 9) from the table of cm2_jump_find
 *   with the same capacity.  d_out may be d_in itself.  With more jumps than the capacity only the first capacity
 *   ones are applied: the caller has to look at the sum first.
 * The stream-sized calls allocate nothing and do not synchronise.  Refused with CM2_ERR_ARGUMENT, the outputs (and
 * *out) untouched: w outside [1, 256]; nt < 1 or nt >= 2^32 - 1; sizes that are not positive or do not add up to nt;
 * more than 2^18 blocks; NULL pointers (d_flags and d_prev may be NULL); a flag_kind other than 0 or 1 with flags
 * given; min_count outside [1, w]; nsigma not finite or <= 0; capacity < 1; radius outside [0, 256]; an output that
 * overlaps an input or another output, except d_out == d_in in cm2_jump_correct. */
#define CM2_JUMP_MAX_WINDOW 256
#define CM2_JUMP_MAX_RADIUS 256
#define CM2_JUMP_CLEAN 0
#define CM2_JUMP_AT 1
#define CM2_JUMP_NEAR 2
typedef struct cm2_jump cm2_jump;
int cm2_jump_create(cm2_jump **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, int half_window,
                    void *stream);
int cm2_jump_destroy(cm2_jump *h);
int cm2_jump_info(const cm2_jump *h, int64_t *h_info);
int cm2_jump_stat(cm2_jump *h, const double *d_in, const void *d_flags, int flag_kind, const uint8_t *d_prev,
                  int min_count, double *d_t, uint8_t *d_noeval, void *stream);
int cm2_jump_scale(cm2_jump *h, const double *d_t, const uint8_t *d_noeval, double *d_sigma, void *stream);
int cm2_jump_find(cm2_jump *h, const double *d_t, const uint8_t *d_noeval, const double *d_sigma, double nsigma,
                  int64_t capacity, int64_t *d_pos, double *d_heights, double *d_offsets, int64_t *d_njumps,
                  void *stream);
int cm2_jump_correct(cm2_jump *h, const double *d_in, const uint8_t *d_prev, const int64_t *d_pos,
                     const double *d_offsets, const int64_t *d_njumps, int64_t capacity, int radius, double *d_out,
                     uint8_t *d_class, int64_t *d_counts, void *stream);

/* ---- f2g: PCA filter  (PCAFilterLO) ------------------------------------------------------------
 * Removes modes across the detectors that are learnt from the data and change from chunk to chunk: the
 * detector-detector covariance of a stretch of data, its leading eigenvectors as the templates, and f2d's fit and
 * removal of them sample by sample.  The eigenproblem is the caller's (PCAFilterLO.learn solves it on the host);
 * the library computes the covariance and applies modes it is given.  No counterpart in the reference.
 * Layout as in f2d: nt = ndet ns, sample i of detector k at k ns + i, flagged where d_pix[nt] < 0, the group edges
 * 0 = g_0 < ... < g_G = ndet.  New here are the chunk edges 0 = c_0 < ... < c_C = ns, and 1 <= K <= CM2_PCA_MAX_K.
 *
 * Covariance, one unit per (chunk c, group g), n = g_{g+1} - g_g detectors a, b counted from g_g:
 *     x[a, i] = d[(g_g + a) ns + i], or +0.0 where d_flags is given and d_flags[(g_g + a) ns + i] < 0
 *     (d_flags NULL: every sample is used; a flagged sample's value is never read),
 *     Cov_u[a n + b] = sum_{i = c_c}^{c_{c+1} - 1} x[a, i] x[b, i].
 * Units are stored chunk-major, then by group: off(c, g) = c sum_g n_g^2 + sum_{g' < g} n_g'^2; cm2_pca_cov_doubles is
 * C sum_g n_g^2.  Stored entries are exactly symmetric: entry (a, b) with a >= b is formed and (b, a) is its copy.
 * Order (no floating-point atomics; the bits do not depend on the run, on ns, on the other chunks or on the other
 * groups, only on the unit's own samples and on the chunk's length): the chunk is cut, from its own first sample,
 * into segments of CM2_PCA_SEGMENT samples (the last one shorter).  Within a segment an entry is one accumulator that
 * starts at +0.0 and takes one v_mfma_f64_16x16x4_f64 per four consecutive samples, in ascending i (the last
 * instruction of a segment is padded with +0.0 samples); how the four products of one instruction are added to the
 * accumulator is the hardware's.  The entry is then p_0 + p_1 + ... + p_{S-1}, the segment partials added from left
 * to right.  Rows beyond the group (the 128-row tiles and 16-row MFMA blocks are padded with +0.0 rows) are never
 * stored.  A non-finite used sample of detector a makes row and column a of its own unit non-finite and nothing
 * else.  A unit whose samples are all flagged is exactly 0.
 *
 * Modes: Phi_c[k, 0..K-1] per chunk and detector, d_modes[(c ndet + k) K + j].
 *
 * Apply, one unit per (group, time sample i), i in chunk c: exactly f2d's unit with Phi = Phi_c.  Gram sums
 * G_ab += Phi_ka Phi_kb, b_a += Phi_ka v[k, i] over the unflagged detectors of the group in ascending k; cm2_fit.h's
 * factor, its pivot rule with tau = CM2_PCA_TAU = 2^-10 and its two solves; the projection
 * out[k, i] = v[k, i] - (((c_0 Phi_k0 + c_1 Phi_k1) + ...) + c_{K-1} Phi_k,K-1) in ascending j; flagged samples and
 * every sample of a skipped unit are 0; the classes are CM2_PCA_FITTED, _EMPTY (m = 0), _FEW (0 < m < K) and _PIVOT.
 * Every product and sum is rounded on its own (-ffp-contract=off).  Given fixed modes the operator is
 * M - M Phi (Phi^T M Phi)^-1 Phi^T M sample by sample: symmetric and idempotent.  With modes learnt from d itself
 * the stage as a whole is not linear in d.
 *
 * cm2_pca_create keeps d_pix (it must not change or be freed while the handle lives) and copies the edges; builds the
 *   work-item and slab tables and the covariance workspace.  Allocates and synchronises.  No modes are set yet.
 * cm2_pca_info: h_info[13] = ns, ndet, ngroups, nchunks, K, covariance doubles, workspace doubles, covariance work
 *   items, 1 when modes are set, units fitted, empty, few, pivot (0 before modes are set).
 * cm2_pca_cov_doubles: the doubles cm2_pca_cov writes (-1 for a NULL handle).
 * cm2_pca_cov: d_cov = the covariances of d_in; d_flags NULL or nt int32.  Two launches in the handle's own
 *   workspace, no allocation, no synchronisation.  Two calls on one handle must not run at the same time.
 * cm2_pca_set_modes copies d_modes[nchunks ndet K], classes every unit and counts the classes.  Synchronises.
 *   Refused when a group has fewer than K + 1 detectors (K modes on K detectors would remove everything); the
 *   covariance of such a handle is still available.
 * cm2_pca_apply: d_out = F d_in (nt doubles each).  One launch, no allocation, no synchronisation.  d_out may be d_in
 *   itself (a thread reads its column before it stores and touches no other); any other overlap is refused.
 * cm2_pca_fit: d_coeff[(g K + j) ns + i] = c_j of unit (g, i), 0 for a skipped unit: the mode time streams.
 * cm2_pca_status: d_status[g ns + i] = the class of unit (g, i), one byte each.  Synchronises.
 * Refused with CM2_ERR_ARGUMENT, the outputs (and *out) untouched: K outside [1, 10]; ns, ndet, ngroups or nchunks
 * < 1; group edges that do not ascend strictly from 0 to ndet; chunk edges that do not ascend strictly from 0 to ns;
 * modes for a handle with a group of fewer than K + 1 detectors; NULL pointers (but d_flags); sizes that overflow the index types or a grid
 * (ndet ns > 2^46, ndet > 2^23, nchunks > 2^16, 2^31 or more workgroups in a launch); d_cov sharing memory with d_in
 * or d_flags; d_out overlapping d_in without being d_in; d_coeff sharing memory with d_in; apply, fit or status
 * before modes are set. */
#define CM2_PCA_TAU 0.0009765625            /* 2^-10 */
#define CM2_PCA_MAX_K 10
#define CM2_PCA_SEGMENT 4096
#define CM2_PCA_FITTED 0
#define CM2_PCA_EMPTY 1
#define CM2_PCA_FEW 2
#define CM2_PCA_PIVOT 3
typedef struct cm2_pca cm2_pca;
int cm2_pca_create(cm2_pca **out, int64_t ns, int ndet, int ngroups, const int64_t *h_group_edges, int64_t nchunks,
                   const int64_t *h_chunk_edges, int K, const int32_t *d_pix, void *stream);
int cm2_pca_destroy(cm2_pca *h);
int cm2_pca_info(const cm2_pca *h, int64_t *h_info);
int64_t cm2_pca_cov_doubles(const cm2_pca *h);
int cm2_pca_cov(cm2_pca *h, const double *d_in, const int32_t *d_flags, double *d_cov, void *stream);
int cm2_pca_set_modes(cm2_pca *h, const double *d_modes, void *stream);
int cm2_pca_apply(cm2_pca *h, const double *d_in, double *d_out, void *stream);
int cm2_pca_fit(cm2_pca *h, const double *d_in, double *d_coeff, void *stream);
int cm2_pca_status(const cm2_pca *h, uint8_t *d_status);

/* ---- f2h: demodulation and decimation  (Demodulator, demodulate, decimate, lowpass_taps) ----------
 * Lock-in demodulation of a stream modulated by a rotating half-wave plate: the stream and its products with the
 * polarisation carrier cos 2 phi, sin 2 phi (cm2_pointing_expand writes it) are low-passed by a FIR filter and one
 * sample in D is kept, which gives three slow streams T, Q, U that map with a plain pol = 1 pointing.  Without a
 * carrier the same kernel decimates.  No counterpart in the reference: the definition is the one below, and every
 * result has the bits it gives, on every run and every layout of threads.
 * Inputs: d[nt]; noise blocks of sizes[0..nblocks-1] samples adding up to nt (BlockLO's convention), block b the n_b
 * samples [start_b, end_b); the factor 1 <= D <= CM2_DEMOD_MAX_FACTOR; the taps h[0..L-1], L odd, 1 <= L <=
 * CM2_DEMOD_MAX_TAPS, c = (L - 1) / 2, every tap finite, Wfull = the taps added from 0.0 in ascending k finite and > 0;
 * optional flags in the two encodings of cm2_gaps_create (flag_kind 0: int32, flagged when negative; 1: bytes, flagged
 * when non-zero; d_flags NULL: nothing flagged); optionally the carrier cosv[nt], sinv[nt]; min_weight in (0, 1].
 * Everything is cut at the block boundaries.  Every operation on doubles named below is rounded once (no fused
 * multiply-add).
 * Outputs: block b gives m_b = ceil(n_b / D) outputs, output j centred on sample j D of the block; the output streams
 * are the blocks one after the other, M = sum m_b.
 *  1. usable_i: the sample is not flagged and d_i is finite.  cosv and sinv are used only at usable samples: what
 *     they hold elsewhere (a NaN) changes nothing.  (They may be loaded there: both arrays are nt doubles.)
 *  2. The terms of output j of block b: k = 0 .. L - 1 in ascending order, i = j D - c + k counted from start_b.  A
 *     term is included when 0 <= i < n_b and sample i is usable.
 *  3. The chains: sT = sQ = sU = W = 0.0; for each included term, in this association,
 *         sT = sT + h_k d_i,  sQ = sQ + h_k (d_i cosv_i),  sU = sU + h_k (d_i sinv_i),  W = W + h_k.
 *     (An excluded term may be added as h_k 0.0 = +-0.0: a chain that started at +0.0 never holds -0.0, so its bits do
 *     not change.  A unit with every term included has W = Wfull, the same additions.)
 *  4. Weight test: W >= min_weight Wfull (one multiplication; false for a NaN).  Passed: T_j = sT / W,
 *     Q_j = 2.0 (sQ / W), U_j = 2.0 (sU / W).  Failed: T_j = Q_j = U_j = +0.0.
 *  5. The class byte: CM2_DEMOD_FULL when all L terms were included; otherwise CM2_DEMOD_PARTIAL when the weight test
 *     passed; otherwise CM2_DEMOD_REJECTED.  counts[b][3], int64: the outputs of block b per class.
 *  6. Without a carrier only T, the classes and the counts exist.
 * Truncated windows bias the result by far more than W / Wfull suggests (the carrier is no longer averaged over whole
 * periods): PARTIAL outputs are for inspection, maps should take FULL ones (cm2_demod_pick with drop_from = 1).  Gaps
 * should be filled (cm2_gaps_fill_linear, GapFiller) before demodulating: a normalised sum across a gap leaks
 * intensity into Q and U.
 *
 * cm2_demod_create copies h_sizes and h_taps; the handle owns the block tables of the input units and the output
 *   prefix, and the taps on the device.  Allocates and synchronises.
 * cm2_demod_info: h_info[9] = nt, nblocks, D, L, M, input samples per workgroup, outputs per thread, LDS bytes of a
 *   workgroup with a carrier, bytes owned.
 * cm2_demod_run: d_T[M], d_class[M] (one byte each), d_counts[nblocks][3] and, with a carrier (d_cos and d_sin both
 *   given), d_Q[M] and d_U[M]; without one d_cos, d_sin, d_Q and d_U are all NULL.  One memset and one launch, no
 *   allocation, no synchronisation.
 * cm2_demod_pick: d_out[M] (int32) = d_pix[centre sample of the output], or -1 where d_class >= drop_from (1: keep
 *   FULL only; 2: keep FULL and PARTIAL) or the centre pixel is negative.  One launch.
 * Refused with CM2_ERR_ARGUMENT, the outputs (and *out) untouched: D outside [1, 64]; nt < 1 or nt >= 2^32 - 1; sizes
 * that are not positive or do not add up to nt; more than 2^18 blocks; an even L, L outside [1, 1025]; a tap that is
 * not finite; Wfull not finite or <= 0; NULL pointers (d_flags may be NULL; the carrier and Q, U as above); a
 * flag_kind other than 0 or 1 with flags given; min_weight outside (0, 1]; drop_from other than 1 or 2; an output that
 * overlaps an input or another output. */
#define CM2_DEMOD_MAX_FACTOR 64
#define CM2_DEMOD_MAX_TAPS 1025
#define CM2_DEMOD_FULL 0
#define CM2_DEMOD_PARTIAL 1
#define CM2_DEMOD_REJECTED 2
typedef struct cm2_demod cm2_demod;
int cm2_demod_create(cm2_demod **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, int factor,
                     const double *h_taps, int ntaps, void *stream);
int cm2_demod_destroy(cm2_demod *h);
int cm2_demod_info(const cm2_demod *h, int64_t *h_info);
int cm2_demod_run(cm2_demod *h, const double *d_in, const double *d_cos, const double *d_sin, const void *d_flags,
                  int flag_kind, double min_weight, double *d_T, double *d_Q, double *d_U, uint8_t *d_class,
                  int64_t *d_counts, void *stream);
int cm2_demod_pick(const cm2_demod *h, const int32_t *d_pix, const uint8_t *d_class, int drop_from, int32_t *d_out,
                   void *stream);

/* ---- f2i: template filter  (TemplateFilterLO) --------------------------------------------------
 * Fits and removes time-domain templates given by the caller, per detector and chunk: a stage thermometer, the air
 * mass 1 / sin(el) (the fitted coefficient of an elevation nod is the relative gain), accelerometer and encoder
 * channels, a scan-synchronous template sampled in time.  It is f2c with the harmonic table replaced by
 * d_templates[J][ns], J = ntemplates, shared by all detectors.  No counterpart in the reference: the definition is the
 * one below.
 * Layout, flags, chunk edges and units as in f2c.  K = J + 1 with the constant (add_constant = 1), K = J without
 * (add_constant = 0); 1 <= K <= CM2_TEMPLATE_MAX_K.
 *     With the constant:    T_0 = 1,  T_j(t) = d_templates[j - 1][t] - mu_{j,c}   (j = 1..J, t in chunk c),
 *     without it:           T_j(t) = d_templates[j][t]                            (j = 0..J-1), as given.
 * mu_{j,c} is the mean of template j over the finite values of ALL samples of chunk c.  The flags do not enter: they
 * differ by detector, the table does not.  Centring does not change out (the constant spans the difference); it is
 * there for the skip rule: a thermometer reading 0.1 K +- 1e-5 is collinear with the constant to 1e-8 and would fail
 * the pivot test in every unit.  c_0 is therefore the offset AT THE CHUNK MEAN of the templates, not at template
 * value 0; the other coefficients are those of the templates as given.
 * Per unit, V its unflagged samples and m = |V|: G, b, c = G^-1 b and out as in f2c,
 *     out_t = v_t - T(t)^T c on V,  out_t = 0 on the flagged samples of the unit
 * (M - M T G^-1 T^T M: symmetric and idempotent).
 * A unit is SKIPPED -- every sample of it 0 in the output, its K coefficients 0 -- when m < K (mark 1), or when the
 * Cholesky factorisation meets a pivot that fails !(p_j > CM2_TEMPLATE_TAU G_jj) (mark 2): two templates equal on
 * the chunk, a template constant on a chunk next to the constant.  A non-finite template value on an unflagged sample
 * of a unit makes G non-finite, the pivot test fails and the unit is skipped with mark 2: this falls out of the test as
 * written and takes no extra pass.  A non-finite template value on samples that are flagged for a detector has no
 * effect on that detector's unit.  A non-finite v_t on an unflagged sample makes its own unit's output non-finite and
 * no other unit's.
 *
 * G depends on the templates and the flags only: it is formed and factorised on the device by cm2_template_create.
 * The handle holds its own copy of the table, centred (J ns doubles, the only state of that size: the caller's array
 * may go away), the factors (K (K + 1) / 2 doubles per unit), the marks and the segment sums of one application
 * (K doubles per segment).
 *
 * Order of the sums (no floating-point atomics; the same bits every time), per detector that of f2c: segments of 4096
 * samples, thread t adds T_j(q) v_q over its unflagged samples q = t, t + 256, ... in ascending order, starting from
 * 0; the 64 lanes of a wave by x += x[lane + off], off = 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3;
 * a unit's segments in ascending order, starting from 0.  The Gram sums are formed the same way; m is an integer
 * count.  mu_{j,c}: thread t of one workgroup adds the finite x_q, q = t, t + 256, ... of the whole chunk in ascending
 * order, starting from 0; lanes and waves as above; mu = sum / (number of finite values), 0 when there is none;
 * T = x - mu.  Then the two triangular solves as in f2c and
 * out_t = v_t - (((c_0 T_0 + c_1 T_1) + c_2 T_2) + ... + c_{K-1} T_{K-1}), where c_0 T_0 is c_0 with the constant.
 * Every product and sum is rounded on its own.  A workgroup works on one segment of several consecutive detectors
 * at once, so that a template value is loaded once for all of them (8 K / Dt bytes per detector sample and pass,
 * Dt = 4 for K <= 2 and 2 above); no sum depends on that grouping.
 *
 * cm2_template_create keeps d_pix (it must not change or be freed while the handle lives) and copies d_templates
 *   (device memory, J ns doubles; may be NULL when J = 0) and h_edges[nchunks + 1].  Allocates and synchronises.
 * cm2_template_info: h_info[10] = ns, ndet, nchunks, K, add_constant, units fitted, units skipped for m < K, units
 *   skipped for a pivot, segment size, segments.
 * cm2_template_apply: d_out = F d_in (nt doubles each).  Three launches, no allocation, no synchronisation.  One handle
 *   runs one apply or fit at a time.
 * cm2_template_fit: d_coeff[ndet nchunks K] = the coefficients c of every unit, without the subtract pass.
 * cm2_template_status: d_status[ndet nchunks] = the mark of every unit, one byte each: CM2_TEMPLATE_FITTED,
 *   CM2_TEMPLATE_FEW, CM2_TEMPLATE_PIVOT.  A copy on the stream.
 * cm2_template_tables: copies the handle's table to d_tables[J][ns] (nothing when J = 0).
 * Refused with CM2_ERR_ARGUMENT, the outputs (and *out) untouched: ntemplates < 0; add_constant other than 0 or 1;
 * K outside [1, 16]; ns, ndet or nchunks < 1; edges that do not ascend strictly from 0 to ns; NULL pointers; sizes that
 * overflow the index types (ns >= 2^40, ndet ns > 2^46, 2^31 or more segments or units); d_out or d_coeff sharing
 * memory with d_in. */
#define CM2_TEMPLATE_TAU 0.0009765625       /* 2^-10 */
#define CM2_TEMPLATE_MAX_K 16
#define CM2_TEMPLATE_FITTED 0
#define CM2_TEMPLATE_FEW 1
#define CM2_TEMPLATE_PIVOT 2
typedef struct cm2_template cm2_template;
int cm2_template_create(cm2_template **out, int64_t ns, int ndet, int64_t nchunks, const int64_t *h_edges,
                        int ntemplates, const double *d_templates, int add_constant, const int32_t *d_pix,
                        void *stream);
int cm2_template_destroy(cm2_template *h);
int cm2_template_info(const cm2_template *h, int64_t *h_info);
int cm2_template_apply(cm2_template *h, const double *d_in, double *d_out, void *stream);
int cm2_template_fit(cm2_template *h, const double *d_in, double *d_coeff, void *stream);
int cm2_template_status(const cm2_template *h, uint8_t *d_status, void *stream);
int cm2_template_tables(const cm2_template *h, double *d_tables, void *stream);

/* ---- f2j: Fourier filter per noise block  (FourierFilter, fourier_filter, deconvolve_time_constant,
 *           FourierFilterLO) --------------------------------------------------------------------------
 * Multiplies the transform of every noise block by a response H_b(f): the inverse (or, for simulations, the forward)
 * one-pole response 1 / (1 + 2 pi i f tau_b) of a bolometer, a Butterworth low-pass and high-pass, cos^2 notches and an
 * arbitrary tabulated response, real or complex.  No counterpart in the reference: the definition is the one below.
 * The stage takes no flags: gaps are to be filled beforehand (cm2_gaps_fill_linear, GapFiller).
 * Inputs: d[nt]; noise blocks of sizes[0..nblocks-1] samples adding up to nt (BlockLO's convention), block b the n
 * samples x_0 .. x_{n-1}; the sample rate fs > 0.  Every operation on doubles named below is rounded once (no fused
 * multiply-add).
 *  1. Bad blocks.  A block with any non-finite input sample is bad: every one of its outputs is the quiet NaN
 *     0x7FF8000000000000, written by the unpack kernel (the transform is not left to decide what such a block
 *     holds).  cm2_fourier_info counts the bad blocks of the last apply.  No other block is affected.
 *  2. Trend.  detrend = 0: l = 0.  detrend = 1 (ends): m = min(end_mean, n), 1 <= end_mean <= 1024; a = the mean of
 *     the first m samples, b = the mean of the last m, each formed by one workgroup: thread t adds the samples t,
 *     t + 256, ... of the m in ascending order from 0.0, the 64 lanes of a wave by x += x[lane + off], off = 32, 16,
 *     8, 4, 2, 1, the four waves as ((w0 + w1) + w2) + w3, then one division by m.
 *     l_i = a + ((b - a) i) / (n - 1);  for n = 1, l_0 = a.
 *  3. Length.  L = fft_length(n, pad): the smallest even integer >= max(2, n + pad) whose prime factors all lie in
 *     {2, 3, 5, 7}; 0 <= pad, L <= 2^28.  xt_i = x_i - l_i for i < n and +0.0 for n <= i < L.  (The padding keeps the
 *     circular convolution from wrapping the end of a block onto its start: a high-pass at f_c wants pad >~ fs / f_c.)
 *  4. Response at bin k = 0 .. L/2:  f = (k fs) / L  and  H_b(f) = T g R  with
 *     T: tau_b >= 0 finite, one per block.  tau_b = 0: T = 1.  Otherwise u = ((2 pi) f) tau_b and
 *        mode 0 (deconvolve): T = 1 + i u;  mode 1 (convolve): T = 1 / (1 + u u) - i u / (1 + u u).
 *     g = 1, then multiplied in this order by
 *        G_lp = 1 / sqrt(1 + w), r = (f / f_lp)^2, w = r multiplied p - 1 times by r, 1 <= p <= 16; absent for f_lp = 0;
 *        G_hp = 0 at k = 0, otherwise the same with r = (f_hp / f)^2 and the order q; absent for f_hp = 0;
 *        G_notch,j for j = 0 .. J - 1, J <= 16, from (f0_j, w_j > 0): a = |f - f0_j| / w_j; sin^2((pi / 2) a) where
 *        a < 1 and exactly 1 elsewhere.
 *     H = (Re T g, Im T g), then times R when a table is given: Rn >= 2 values shared by all blocks (table_per_block
 *        0, [Rn]) or per block (1, [nblocks][Rn]) on the grid f_r = r (fs / 2) / (Rn - 1), real (table_kind 1) or
 *        complex (table_kind 2, re and im interleaved), all finite; s = (f / (fs / 2)) (Rn - 1), r = min(floor s,
 *        Rn - 2), t = s - r, R = R_r + t (R_{r+1} - R_r) in the real and in the imaginary part.  A real R scales both
 *        parts of H; a complex one multiplies as (re re - im im, re im + im re).
 *     conjugate = 1 replaces H by its conjugate: the transposed operator (for detrend = 0).
 *     At k = 0 and k = L/2 the imaginary part of H is set to +0.0.  (The transform of a real stream is real there.
 *     Convolve followed by deconvolve on an unpadded block is therefore the identity at every bin but the Nyquist
 *     one, which keeps the factor 1 / (1 + u u).)
 *  5. Output.  y_i = (1/L) sum_k H_b(f_k) Xt_k e^{2 pi i i k / L}, the real inverse transform of the product (the
 *     unnormalised inverse divided by L), for i < n, and out_i = y_i + Re H_b(0) l_i (detrend = 0: out_i = y_i).
 *     The trend goes through the filter as a constant would: the constant tau slope fs that a deconvolved ramp would
 *     carry is NOT restored.
 * The transforms are rocFFT's: the result is the definition's to rounding (tests/_fourier_ref.py has the bound), and
 * has the same bits run to run (no floating-point atomics).
 *
 * cm2_fourier_create copies h_sizes, h_tau[nblocks] (NULL: every tau 0), h_notch[J][2] and the table.  It groups the
 *   blocks by L (at most 8 distinct lengths) and makes one plan per length for a batch of rows, one row = one block:
 *   L doubles and L/2 + 1 double2.  A batch is at most 2^24 / L rows and at most what max_work_bytes (<= 0: 512 MB)
 *   holds together with the plan's own work buffer; it is halved until that fits, and a single row that does not fit
 *   is refused with the bytes it needs.  The rows are shared by all lengths.  Allocates and synchronises.
 * cm2_fourier_apply: d_out[nt] = F d_in[nt]; d_out may be d_in itself.  No allocation, no synchronisation.  One handle
 *   runs one apply at a time.
 * cm2_fourier_response: d_H[L/2 + 1][2] = H_block as the filter kernel evaluates it, L the length of that block.
 * cm2_fourier_info: h_info[29] = nt, nblocks, number of lengths, bytes of the rows and plans, bad blocks of the last
 *   apply (reads them back: synchronises the stream), then 8 lengths, their 8 batches and their 8 block counts (0
 *   beyond the number of lengths).
 * Refused with CM2_ERR_ARGUMENT, the outputs (and *out) untouched: nt < 1 or nt >= 2^32 - 1; sizes that are not
 * positive or do not add up to nt; more than 2^18 blocks; fs not finite or <= 0; mode or conjugate other than 0, 1; a
 * tau that is negative or not finite; a cut-off that is negative or not finite, an order outside [1, 16]; more than 16
 * notches, an f0 that is not finite, a width that is not finite or <= 0; table_kind outside 0..2, Rn < 2, a table value
 * that is not finite; detrend other than 0, 1; end_mean outside [1, 1024]; pad < 0 or an L beyond 2^28; more than 8
 * lengths; a row that does not fit; NULL pointers (h_tau, h_notch with J = 0 and the table with kind 0 may be NULL);
 * a block outside [0, nblocks); d_out overlapping d_in other than being d_in. */
#define CM2_FOURIER_DECONVOLVE 0
#define CM2_FOURIER_CONVOLVE 1
#define CM2_FOURIER_MAX_ORDER 16
#define CM2_FOURIER_MAX_NOTCH 16
#define CM2_FOURIER_MAX_END_MEAN 1024
#define CM2_FOURIER_MAX_LENGTHS 8
typedef struct cm2_fourier cm2_fourier;
int cm2_fourier_create(cm2_fourier **out, int64_t nt, const int64_t *h_sizes, int64_t nblocks, double fs,
                       const double *h_tau, int mode, double f_lp, int p, double f_hp, int q, const double *h_notch,
                       int nnotch, const double *h_table, int64_t Rn, int table_kind, int table_per_block, int detrend,
                       int end_mean, int64_t pad, int conjugate, int64_t max_work_bytes, void *stream);
int cm2_fourier_destroy(cm2_fourier *h);
int cm2_fourier_info(const cm2_fourier *h, int64_t *h_info, void *stream);
int cm2_fourier_apply(cm2_fourier *h, const double *d_in, double *d_out, void *stream);
int cm2_fourier_response(const cm2_fourier *h, int64_t block, double *d_H, void *stream);

/* ---- f3: solution vector <-> full-sky HEALPix maps -------------------------------
 * cm2_cutsky_to_fullsky: d_full is pol arrays of nfull doubles one after the other
 * ([I | Q | U]); component k of observed pixel i, d_map[pol*i + k], goes to
 * d_full[k*nfull + d_obspix[i]], all other pixels are 0 (reorganize_map,
 * utilities/healpy_functions.py:47-102).  cm2_fullsky_to_cutsky is the inverse gather
 * (full2cutskymap, utilities/IOfiles.py:377-393).  Pixel ids outside [0, nfull) fail, before anything is written. */
int cm2_cutsky_to_fullsky(int pol, int64_t npix, const int64_t *d_obspix, const double *d_map,
                          int64_t nfull, double *d_full, void *stream);
int cm2_fullsky_to_cutsky(int pol, int64_t npix, const int64_t *d_obspix, const double *d_full,
                          int64_t nfull, double *d_map, void *stream);

/* ---- n1: inverse-noise bands estimated from the time streams ---------------------
 * The reference has no estimator; its ToeplitzLO (linearoperators.py:582-595) defines what a band
 * means.  L = nperseg is a power of two in [256, 65536].
 *
 * cm2_psd_welch: Welch PSD of each block of the TOD d_tod (blocks of h_sizes[0..nb-1] samples, one
 * after the other, each >= L), d_psd[b][k] for k = 0..L/2 -- scipy.signal.welch(x_b, fs, window='hann',
 * nperseg=L, noverlap=L/2, detrend='constant' (detrend = 1) or False (0), scaling='density',
 * average='mean'); block b has K_b = (n_b - L) / (L/2) + 1 segments, a tail that does not fill one is
 * ignored, and the per-bin sum of |X_s(k)|^2 runs in segment order.  Sample offsets are 64-bit.
 * The work runs over batches of a fixed number of segments, set at cm2_psd_create from L and
 * max_work_bytes (<= 0: 512 MB; the batch is at least one segment, whatever the cap), so that the
 * result of a block does not depend on the other blocks of the call: bit-equal to the same block
 * estimated alone.  Overwrites d_psd; synchronises.  One handle must not run two calls at once.
 * cm2_psd_info: h_info[3] = L, segments per batch, workspace bytes of the handle. */
typedef struct cm2_psd cm2_psd;
int cm2_psd_create(cm2_psd **out, int64_t nperseg, int detrend, int64_t max_work_bytes, void *stream);
int cm2_psd_destroy(cm2_psd *p);
int cm2_psd_info(const cm2_psd *p, int64_t *h_info);
int cm2_psd_welch(cm2_psd *p, const double *d_tod, const int64_t *h_sizes, int64_t nb,
                  double fsample, double *d_psd, void *stream);
/* d_bands[b][0..lambda-1] (1 <= lambda <= L/2) from the one-sided PSD d_psd[b][0..L/2]:
 * S_k = P_k fs / m_k (m_k = 1 at k = 0 and L/2, else 2), S_0 := S_1, G = 1/S,
 * c_j = irfft(G, L)[j] as a cosine sum over k in increasing order, a_j = (1 - j/lambda) c_j (Bartlett:
 * the band's symbol is G smoothed by the Fejer kernel, so every block is SPD).  A bin with S <= 0 or
 * not finite, or so small that 1/S overflows, fails with CM2_ERR_ARGUMENT and a message naming the block
 * and the bin (the first in block-major order; d_bands is then left untouched).  Overwrites d_bands;
 * synchronises. */
int cm2_noise_bands_from_psd(const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                             int64_t lambda, double *d_bands, void *stream);

/* ---- n2: noise time streams drawn from a PSD --------------------------------------
 * The reference has no simulator.  Everything is a function of (seed, realization, block, sample index)
 * alone: grid sizes, call boundaries, the device and the way a TOD is sharded do not change a sample.
 *
 * cm2_rng_fill: d_out[0..n) = samples first .. first+n-1 (first, n >= 0) of the white stream
 * (seed, realization, block): Philox4x64-10 with key [seed, realization]; output block j = 0, 1, ... (four
 * uint64) is the Philox function of the counter [j + 1, block, 0, 0], i.e.
 * numpy.random.Philox(key=[seed, realization], counter=[0, block, 0, 0]).random_raw() bit for bit.
 *   kind 0  uniform in [0, 1): u = (raw >> 11) 2^-53, bit-equal to numpy.random.Generator(...).random()
 *   kind 1  standard normal: Box-Muller over the pairs (u0, u1) and (u2, u3) of a counter block, samples
 *           4j, 4j+1 from the first and 4j+2, 4j+3 from the second: r = sqrt(-2 log(1 - u_a)),
 *           z_a = r cospi(2 u_b), z_b = r sinpi(2 u_b)  (1 - u_a is in (0, 1]: the logarithm never sees 0).
 * Counter blocks cut by `first` or `first + n` are generated whole and masked.  Does not synchronise. */
int cm2_rng_fill(int kind, uint64_t seed, uint64_t realization, uint64_t block, int64_t first, int64_t n,
                 double *d_out, void *stream);
/* The colouring band: cm2_noise_bands_from_psd with G = sqrt(S) in place of 1/S, g_j = (1 - j/lambda)
 * irfft(sqrt(S), L)[j].  The symbol g^(w) = g_0 + 2 sum_j g_j cos(w j) is sqrt(S) smoothed by the Fejer kernel
 * (>= 0), and white noise filtered with g has the spectrum |g^|^2 (S itself up to that resolution).  S = 0 is
 * allowed; a bin with S < 0 or not finite fails with CM2_ERR_ARGUMENT naming the block and the bin. */
int cm2_noise_filter_from_psd(const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                              int64_t lambda, double *d_bands, void *stream);
/* cm2_noise_sim: coloured noise for nblocks blocks of h_sizes[b] samples with the bands h_bands[b][0..lambda-1]
 * (host).  Block b of a draw is
 *     y_i = sum_{|j| < lambda} g_|j| w_{i + (lambda-1) + j},   i = 0 .. n_b - 1,
 * with w the first n_b + 2 (lambda-1) normals (cm2_rng_fill, kind 1) of the stream (seed, realization,
 * first_block + b): the valid part of the convolution, so every sample of the block has the autocovariance
 * g * g, up to the block edges.  Blocks are independent streams: a handle for blocks [k0, k1) of a TOD, made
 * with first_block = k0, draws the samples a handle for the whole TOD draws for those blocks.
 * The handle owns two buffers of sum_b (n_b + 2 (lambda-1)) doubles and a cm2_noise Toeplitz operator
 * (CM2_TOEPLITZ_AUTO) on the padded blocks, whose interior rows are the sum above.
 * cm2_noise_sim_draw: d_out[0..nt) = (add ? d_out : 0) + scale * y.  No allocation, no host copy, does not
 * synchronise; one handle must not run two draws at once.
 * cm2_noise_sim_info: h_info[7] = nt, nblocks, lambda, padded samples, CM2_TOEPLITZ_* method of the
 * operator, its FFT length (0: direct sum), bytes of the two padded buffers. */
typedef struct cm2_noise_sim cm2_noise_sim;
int cm2_noise_sim_create(cm2_noise_sim **out, const double *h_bands, int64_t lambda, const int64_t *h_sizes,
                         int64_t nblocks, uint64_t seed, uint64_t first_block, void *stream);
int cm2_noise_sim_destroy(cm2_noise_sim *s);
int cm2_noise_sim_info(const cm2_noise_sim *s, int64_t *h_info);
int cm2_noise_sim_draw(cm2_noise_sim *s, uint64_t realization, double scale, int add, double *d_out,
                       void *stream);

/* ---- n3: the flagged samples of a time stream, and their fill ---------------------------
 * The reference flags a sample with pix = -1 (flagging_subscan, utilities/IOfiles.py:142-152; the samples of
 * a masked pixel, process_ces.py:403-418) and has no gap filling: P and P^T skip such samples, ToeplitzLO.mult
 * (interfaces/linearoperators.py:582-595) does not.  G = the flagged samples, V = the valid ones, Q = N^-1.
 *
 * cm2_gaps_create: d_flags holds nt flags, flag_kind 0 = int32 (flagged when negative: the pix array),
 * 1 = bytes (flagged when non-zero).  The handle KEEPS d_flags: the caller keeps the buffer alive and
 * unchanged.  Noise blocks of h_sizes[0..nblocks-1] samples (adding up to nt < 2^32 - 1; positions are stored
 * as uint32).  The handle owns ng and the ascending positions of the flagged samples (a hipCUB select, no sort)
 * and the table of runs of consecutive flagged samples, cut at the block boundaries.  With h_a0 (a_0 of every
 * block's band, > 0) it also owns the compact Jacobi vector 1 / a_0(block of the sample) and two buffers of nt
 * doubles: the scatter target (zeroed here, only its ng flagged positions are ever written again) and the output
 * of N^-1; h_a0 == NULL makes a handle for cm2_gaps_fill_linear, gather and scatter only.  Synchronises.
 * cm2_gaps_info: h_info[5] = nt, ng, runs, longest run, bytes of the two buffers.
 * cm2_gaps_index: h_pos[ng] = the positions (may be NULL), h_runs[3 runs] = (start, length, block) of every run
 * (may be NULL).  Synchronises.
 * "Compact" vectors hold ng doubles, the flagged samples in time order. */
typedef struct cm2_gaps cm2_gaps;
int cm2_gaps_create(cm2_gaps **out, const void *d_flags, int flag_kind, int64_t nt, const int64_t *h_sizes,
                    int64_t nblocks, const double *h_a0, void *stream);
int cm2_gaps_destroy(cm2_gaps *g);
int cm2_gaps_info(const cm2_gaps *g, int64_t *h_info);
int cm2_gaps_index(const cm2_gaps *g, uint32_t *h_pos, int64_t *h_runs, void *stream);
/* d_compact[j] = d_stream[position j];  d_stream[position j] = d_compact[j] (the valid samples of d_stream are
 * not touched).  Do not synchronise. */
int cm2_gaps_gather(const cm2_gaps *g, const double *d_stream, double *d_compact, void *stream);
int cm2_gaps_scatter(const cm2_gaps *g, const double *d_compact, double *d_stream, void *stream);
/* d_out = Q_GG d_y on compact vectors, (N^-1 scatter(y))_G with `noise` a Toeplitz operator on the same blocks:
 * scatter into the handle's zero stream, cm2_noise_apply, gather -- one time-order N^-1 plus 2 ng doubles and
 * 2 ng positions of traffic, no allocation, no synchronisation.  One handle must not run two at once.
 * cm2_gaps_precond_apply: d_z = d_r / a_0(block), cm2_xmy with the compact Jacobi vector. */
int cm2_gaps_normal_apply(cm2_gaps *g, cm2_noise *noise, const double *d_y, double *d_out, void *stream);
int cm2_gaps_precond_apply(const cm2_gaps *g, const double *d_r, double *d_z, void *stream);
/* d_u[i] = 0 where flagged, d_n[i] - d_d[i] elsewhere (d_n == NULL: n = 0), nt doubles in one pass.  A select:
 * what d_d holds at a flagged sample never enters arithmetic that is kept.  d_u is neither input.
 * cm2_gaps_rhs: that, then d_b = (N^-1 u)_G (compact); d_u is nt doubles of scratch. */
int cm2_gaps_masked_diff(const cm2_gaps *g, const double *d_n, const double *d_d, double *d_u, void *stream);
int cm2_gaps_rhs(cm2_gaps *g, cm2_noise *noise, const double *d_n, const double *d_d, double *d_u, double *d_b,
                 void *stream);
/* d_out[i] = d_d[i] on the valid samples (bit for bit; nothing is moved when d_out == d_d), d_n[i] + d_y[j] at
 * the j-th flagged sample (d_n == NULL: n = 0). */
int cm2_gaps_finish(const cm2_gaps *g, const double *d_d, const double *d_n, const double *d_y, double *d_out,
                    void *stream);
/* Linear fill: for each run [s, s + len) inside its block, L = mean of the valid samples among the nedge samples
 * before s inside the block, R = the same for the nedge samples after the run, each summed in time order by one
 * thread; a side without a valid sample takes the other side's level, both without: 0.  d_out[s + k] =
 * L + (R - L) (k + 1) / (len + 1); valid samples are copied bit for bit (d_out == d_d: left where they are).
 * nedge >= 1; a value above nt means nt. */
int cm2_gaps_fill_linear(const cm2_gaps *g, const double *d_d, double *d_out, int64_t nedge, void *stream);

/* The gap-aware normal operator: one unknown per flagged sample.  With E the nt x ng matrix that has a one at
 * (position of the j-th flagged sample, j) and P_e = [P E],
 *     A_e = P_e^T N^-1 P_e = [ P^T Q P   P^T Q E ]      on vectors z = [map (pol npix) ; g (ng, compact)].
 *                            [ E^T Q P   Q_GG    ]
 * Eliminating g from A_e z = P_e^T N^-1 d0 (d0 = d on V, 0 on G) leaves (P^T S P) m = P^T S d_V with the Schur
 * complement S = Q_VV - Q_VG Q_GG^-1 Q_GV, the GLS map of the valid samples alone; g = Q_GG^-1 Q_GV (d_V - P m).
 * A tile-order stream has no slot for a flagged sample, so on a tile plan the chain goes through the time order:
 * cm2_P_tiles_apply, tile -> time order with g written into the flagged samples, cm2_noise_apply, time -> tile
 * order with the flagged samples read out, cm2_Pt_tiles_apply.
 *
 * cm2_gaps_prepare_tiles: makes `tiles` the plan of the handle (one at a time, keyed by the plan's id; a call for
 * the plan already prepared returns at once).  Refuses with CM2_ERR_ARGUMENT a plan with another nt, one whose
 * valid samples and the handle's flagged ones do not add up to nt, and one whose flagged set differs (a device pass
 * over the plan's index and the handle's flags; the message names the first sample that differs).  Builds the
 * plan's windowed permutation lists if they do not exist yet and the table of the windows' compact ranges (windows
 * of 8192 time samples; window w owns the flagged samples [c_w, c_{w+1}), c_w = the number of positions below
 * 8192 w).  Allocates and synchronises.  A stream shorter than one window has no table: the per-sample
 * permutations and cm2_gaps_scatter / cm2_gaps_gather serve.
 * cm2_gaps_window_table: *h_nwin = windows of the table (0: none), h_table[nwin + 1] = c_w (may be NULL).
 * cm2_gaps_tiles_to_time: d_time = cm2_tod_tiles_to_time(d_tb) with d_compact written into the flagged samples,
 * in one kernel; cm2_gaps_time_to_tiles: d_tb = cm2_tod_time_to_tiles(d_time), d_compact_out = the flagged samples
 * of d_time.  Both bit-equal to the two-call forms; after prepare no allocation and no synchronisation.
 * cm2_PtNP_gaps_apply: d_out = A_e d_z (pol npix + ng doubles each, d_out != d_z) on `stream`.  Scratch of the
 * caller: d_tb (valid samples of the plan), d_time1 != d_time2 (nt doubles each).  `noise` is a Toeplitz operator
 * on the handle's blocks.  After cm2_gaps_prepare_tiles (and cm2_tiles_prepare_pt): kernel launches only. */
int cm2_gaps_prepare_tiles(cm2_gaps *g, const cm2_tiles *tiles, void *stream);
int cm2_gaps_window_table(const cm2_gaps *g, int64_t *h_nwin, uint32_t *h_table, void *stream);
int cm2_gaps_tiles_to_time(const cm2_gaps *g, const cm2_tiles *tiles, const double *d_tb, const double *d_compact,
                           double *d_time, void *stream);
int cm2_gaps_time_to_tiles(const cm2_gaps *g, const cm2_tiles *tiles, const double *d_time, double *d_tb,
                           double *d_compact_out, void *stream);
int cm2_PtNP_gaps_apply(const cm2_tiles *tiles, cm2_noise *noise, const cm2_gaps *g, const double *d_z,
                        double *d_out, double *d_tb, double *d_time1, double *d_time2, void *stream);

/* ---- n4: destriping -- the baseline-offset templates F and F^T ---------------------------
 * The correlated noise is modelled as one constant ("offset") per baseline.  The stream has noise blocks of
 * h_sizes[0..nblocks-1] samples (adding up to nt < 2^32 - 1); block b = [o_b, o_b + n_b) is cut into
 * K_b = ceil(n_b / L) baselines, baseline (b, k) = [o_b + k L, min(o_b + (k + 1) L, o_b + n_b)) with the global index
 * j = sum of K_b' over b' < b, plus k; na = sum of K_b < 2^31.  A sample is valid when d_pix[t] >= 0; w_b is the
 * weight of block b (h_weights == NULL: 1), w_t = w_b on the valid samples and 0 on the flagged ones.
 *     (F a)_t = a_j(t) on the valid samples, 0 on the flagged ones;   (F^T y)_j = sum of y_t over the valid t of j.
 * `weighted` = 1 multiplies every output once by w_b (W F a, F^T W y: the weight is factored out of the sum), 0 does
 * not.  The summation order of F^T is fixed by (nt, h_sizes, L) alone: windows of 8192 samples counted from t = 0,
 * inside a window a fixed tree over chunks of 32 samples, a baseline's windows added in ascending order through a
 * side buffer of two slots per window; no floating-point atomics.  The time-order and the tile-order forms give the
 * same bits.
 *
 * cm2_offsets_create: the handle KEEPS d_pix (the caller keeps it alive and unchanged) and owns the block table,
 * nvalid_j (counted on the device), wsum_j = w_b nvalid_j and the side buffer.  Refuses with CM2_ERR_ARGUMENT
 * nt >= 2^32 - 1, na >= 2^31, L < 1, sizes that do not add up to nt, weights that are not positive and finite --
 * before the device is touched.  Synchronises.
 * cm2_offsets_info: h_info[8] = nt, nblocks, L, na, valid samples, windows, tile forms (0 not prepared, 1 on the
 * plan's window lists, 2 per sample), LDS bytes of the window kernels.
 * cm2_offsets_counts: h_nvalid[na], h_wsum[na] (either may be NULL).  Synchronises.
 * cm2_offsets_expand:   d_out[t] = [w_b] d_a[j(t)] on the valid samples, 0 on the flagged ones (nt doubles).
 * cm2_offsets_residual: d_out[t] = [w_b] (d_d[t] - d_a[j(t)]) on the valid samples (d_a == NULL: [w_b] d_d[t]), 0 on
 * the flagged ones.  A select: what d_d holds at a flagged sample is loaded and dropped.  d_out may be d_d.
 * cm2_offsets_sum:      d_out[j] = [w_b] (F^T d_y)_j (na doubles).  One handle must not run two sums at once (the
 * side buffer).  None of the three allocates or synchronises.
 *
 * On a tile plan: cm2_offsets_prepare_tiles makes `tiles` the plan of the handle (keyed by the plan's id; a call for
 * the plan already prepared returns at once).  Refuses with CM2_ERR_ARGUMENT a plan with another nt, one with another
 * number of valid samples, and one whose flagged set differs from d_pix's (a device pass; the message names the
 * first sample that differs).  Builds the plan's windowed permutation lists if they do not exist yet; a stream
 * shorter than one window has none, and the handle then keeps nt doubles for the per-sample permutations.
 * Allocates and synchronises.
 * cm2_offsets_to_tiles:   d_tb = cm2_tod_time_to_tiles(cm2_offsets_expand(d_a)) in one kernel, bit for bit.
 * cm2_offsets_from_tiles: d_out = cm2_offsets_sum(cm2_tod_tiles_to_time(d_tb)) in one kernel (and the combine),
 * bit for bit.  After prepare: kernel launches only. */
typedef struct cm2_offsets cm2_offsets;
int cm2_offsets_create(cm2_offsets **out, const int32_t *d_pix, int64_t nt, const int64_t *h_sizes, int64_t nblocks,
                       int64_t baseline_length, const double *h_weights, void *stream);
int cm2_offsets_destroy(cm2_offsets *f);
int cm2_offsets_info(const cm2_offsets *f, int64_t *h_info);
int cm2_offsets_counts(const cm2_offsets *f, int64_t *h_nvalid, double *h_wsum, void *stream);
int cm2_offsets_expand(const cm2_offsets *f, const double *d_a, int weighted, double *d_out, void *stream);
int cm2_offsets_residual(const cm2_offsets *f, const double *d_d, const double *d_a, int weighted, double *d_out,
                         void *stream);
int cm2_offsets_sum(cm2_offsets *f, const double *d_y, int weighted, double *d_out, void *stream);
int cm2_offsets_prepare_tiles(cm2_offsets *f, const cm2_tiles *tiles, void *stream);
int cm2_offsets_to_tiles(const cm2_offsets *f, const cm2_tiles *tiles, const double *d_a, int weighted, double *d_tb,
                         void *stream);
int cm2_offsets_from_tiles(cm2_offsets *f, const cm2_tiles *tiles, const double *d_tb, int weighted, double *d_out,
                           void *stream);
/* The destriper's noise model from a PSD: d_bands[b][0..lambda-1], the first row of the banded-Toeplitz prior
 * C_a^-1 on the offsets of block b, and the white variance sigma_b^2 (the block's weight is w_b = 1 / sigma_b^2),
 * from the row d_psd[b][0..n/2] of a one-sided PSD (cm2_psd_welch), n = nperseg a power of two in [256, 65536],
 * baseline length L >= 1.  Per block:
 *   1. S_k = P_k fs / m_k (m_k = 1 at k = 0 and n/2, else 2), S_0 := S_1, as cm2_noise_bands_from_psd.  A bin with
 *      S <= 0 or not finite fails with CM2_ERR_ARGUMENT and a message naming the block and the bin (the first in
 *      block-major order).
 *   2. sigma^2 = h_sigma2_in[b], positive and finite, or (h_sigma2_in NULL)
 *      sigma^2 = (4/n) sum_{k = n/4}^{n/2 - 1} S_k.
 *   3. R_k = max(S_k - sigma^2, 0), the correlated part.
 *   4. q_j = (1/n) sum_{k = 0}^{n/2} m_k R_k D_k cos(w_k L j), j = 0 .. K-1, K = floor((n/2 + 1) / L),
 *      w_k = 2 pi k / n, D_k = sin^2(L w_k / 2) / (L^2 sin^2(w_k / 2)), D_0 = 1: the covariance of the means of two
 *      baselines j apart, (1/L^2) sum_{|s| < L} (L - |s|) r_{|jL + s|} with r = irfft(R, n), in closed form; no lag
 *      beyond n/2 is used.  K < 2 is refused (the message gives the smallest nperseg that would do).
 *   5. Q_i = q~_0 + 2 sum_{j = 1}^{K-1} q~_j cos(2 pi i j / M), q~_j = (1 - j/K) q_j, i = 0 .. M/2, M the smallest
 *      power of two >= 2K: the offsets' spectrum, >= 0 by the Bartlett taper (a Fejer-smoothed symbol).
 *   6. H_i = 1 / max(Q_i, floor sigma^2 / L), floor in (0, 1]: sigma^2 / L is the white variance of a baseline
 *      mean, so the prior is bounded by wsum / floor.
 *   7. band_i = (1 - i/lambda) (1/M) sum_{k = 0}^{M/2} m'_k H_k cos(2 pi i k / M), i = 0 .. lambda-1,
 *      1 <= lambda <= M/2, m' like m on M: the second Bartlett taper makes every block SPD.
 *   8. Every sum runs in increasing index order in one accumulator; the angles are reduced in integers before
 *      cospi / sinpi.  A block gives the same bits alone and inside a group.
 * A short last baseline of a block, or one with flagged samples, is treated like a full one.
 * Every bad argument is refused before the device is touched.  Overwrites d_bands[nb][lambda] and, when it is not
 * NULL, h_sigma2_out[nb] (host); synchronises. */
int cm2_offset_prior_from_psd(const double *d_psd, int64_t nb, int64_t nperseg, double fsample,
                              int64_t baseline_length, int64_t lambda, const double *h_sigma2_in /* NULL: estimate */,
                              double floor, double *d_bands, double *h_sigma2_out /* may be NULL */, void *stream);

/* Pointing expansion: one boresight quaternion per time sample and one offset quaternion per detector ->
 * d_pix[k ns + i], d_cos[k ns + i], d_sin[k ns + i] (detector-major), the arrays cm2_pointing_create,
 * cm2_tiles_create and cm2_gaps_create read.  Quaternions are (x, y, z, w), scalar last, Hamilton product; every
 * operation in IEEE double in the order written, nothing contracted:
 *   1. q = (q_frame q_bore[i]) q_det[k] (without a frame: q_bore[i] q_det[k]), each component of a product p q
 *      summed left to right:  x = pw qx + px qw + py qz - pz qy,  y = pw qy - px qz + py qw + pz qx,
 *      z = pw qz + px qy - py qx + pz qw,  w = pw qw - px qx - py qy - pz qz.
 *   2. n2 = ((xx + yy) + zz) + ww, r = 1 / n2: the one normalisation.
 *      d = R(q) z^ = ((2 (x z + w y)) r, (2 (y z - w x)) r, ((ww + zz) - (xx + yy)) r), the line of sight;
 *      o = R(q) x^ = (((ww + xx) - (yy + zz)) r, (2 (x y + w z)) r, (2 (x z - w y)) r), the sensitive direction.
 *   3. The pixel is the HEALPix pixel of d (Gorski et al. 2005, ApJ 622, 759), nside a power of two <= 8192
 *      (12 nside^2 < 2^31), RING (nest = 0) or NESTED: z = dz, t = atan2(dy, dx) (2/pi) wrapped into [0, 4)
 *      (t < 0: t += 4; t >= 4: t -= 4).  |z| <= 2/3: jp = floor(nside (0.5 + t) - (nside z) 0.75),
 *      jm = floor(nside (0.5 + t) + (nside z) 0.75).  Else tmp = nside sqrt(3 (1 - |z|)) while |z| <= 0.99 and
 *      (nside sqrt(dx dx + dy dy)) sqrt(3 / (1 + |z|)) beyond, tp = t - min(3, floor(t)), jp = floor(tp tmp),
 *      jm = floor((1 - tp) tmp), and in RING ordering ip = floor(t (jp + jm + 1)).  The NESTED bit interleave is
 *      shifts and masks.
 *   4. The angle psi is in the COSMO convention, from the local meridian pointing south toward east:
 *      s2 = dx dx + dy dy, a = (ox (z dx) + oy (z dy)) - oz s2, b = oy dx - ox dy (s2 == 0: a = ox z, b = oy, the
 *      meridian of longitude 0), den = a a + b b, cos 2 psi = (a a - b b) / den, sin 2 psi = (2 (a b)) / den
 *      (den == 0: 1, 0).  No transcendental function on this path.
 *   5. d_hwp (plate angle chi[i], rad): phi = psi + 2 chi; (c4, s4) = sincos(4 chi[i]) once per time sample,
 *      cos 2 phi = c c4 - s s4, sin 2 phi = s c4 + c s4.  NULL: phi = psi.
 *   6. Flagged: d_flags[i] != 0, or n2 is not a normal positive finite double (a boresight component that is not
 *      finite, a zero boresight quaternion): pix = -1, cos = 1, sin = 0, the flag convention of every operator here.
 * d_cos and d_sin both NULL: pixels only (pol = 1).  h_frame: 4 doubles on the host, NULL for none.  d_bore must be
 * 16-byte aligned.  CM2_ERR_ARGUMENT, with every output untouched: nside not a power of two in [1, 8192], ndet < 1,
 * ns < 0, exactly one of d_cos / d_sin, a frame quaternion (checked on the host) or a detector quaternion (checked
 * by a kernel before the expansion is launched; the message names the first) whose n2 is not a normal positive
 * finite double.  ns == 0 succeeds and writes nothing.  Synchronises once, on the detector check. */
int cm2_pointing_expand(int64_t ns, int ndet, const double *d_bore /* [ns][4] */,
                        const double *d_detquat /* [ndet][4], detector frame -> boresight frame */,
                        const double *h_frame /* NULL: identity */, const double *d_hwp /* [ns] or NULL */,
                        const uint8_t *d_flags /* [ns] or NULL */, int64_t nside, int nest,
                        int32_t *d_pix /* [ndet ns] */, double *d_cos, double *d_sin /* [ndet ns] or both NULL */,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COSMOMAP2_H */
