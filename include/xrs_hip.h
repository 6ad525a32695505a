/*
 * xrs_hip.h -- C ABI of libxrs_hip.so, the MI355X (gfx950) backend for the dense 2-D
 * raster hot path of xarray-spatial.
 *
 * The reference has no FFI of its own: its only extension seam is the four-slot
 * backend table ArrayTypeFunctionMapping(numpy_func, cupy_func, dask_func,
 * dask_cupy_func) (xrspatial/utils.py:117-143) whose slots are per-backend
 * "runner" functions taking raw arrays.  Each entry point below replaces one such
 * runner (cited per function); the Python host layer (xrspatial_amd/) binds them
 * with ctypes and keeps validation / metadata / Dataset handling above the ABI.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; the message of the
 *    calling thread's last failure is read with xrs_last_error().
 *  - plain pointers and sizes only.  Pointers named *_dev are device (HBM)
 *    pointers obtained from xrs_malloc(); everything else is host memory.
 *  - the caller owns every buffer; the library never allocates outputs, never
 *    frees inputs, and keeps no global mutable state (re-entrant: the reference's
 *    Numba kernels are nogil and may be called from several threads).
 *  - rasters are C-order float32 planes: element (y, x) of a plane `p` with row
 *    pitch `ld` (in ELEMENTS) is p[y * ld + x].  `rows` counts the rows this call
 *    OWNS (and writes); `halo_top` / `halo_bot` say how many extra valid input
 *    rows sit directly above `in_dev` (at negative row indices) / below row
 *    rows-1.  0 means that side is a true raster edge.  This is the row-shard
 *    contract of the multi-GPU path (reference semantics: dask
 *    map_overlap(depth=k//2, boundary=nan), e.g. xrspatial/slope.py:94-97).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *    kernels are asynchronous on it.
 */
#ifndef XRS_HIP_H
#define XRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ runtime */
int xrs_version(void);                                   /* ABI version, currently 1 */
int xrs_last_error(char *buf, size_t buflen);            /* copies the thread's last error text */
/* 16 hex digits identifying the SOURCES this library was built from (sha256 of csrc/ + this header, made by the
 * Makefile): profiles/pmc_traffic.json records the build its counters were collected on and bench.py reports them only
 * for that build. */
int xrs_build_id(char *buf, size_t buflen);
int xrs_device_count(int *count);
int xrs_set_device(int device);
int xrs_get_device(int *device);
int xrs_device_name(int device, char *buf, size_t buflen);
int xrs_mem_info(size_t *free_bytes, size_t *total_bytes);
int xrs_malloc(void **ptr_dev, size_t bytes);
int xrs_free(void *ptr_dev);
/* Page-locked host memory: copies to / from it run at PCIe rate and are truly asynchronous on `stream`
 * (the host layer stages numpy-backed inputs / results through a pool of such blocks). */
int xrs_host_alloc(void **ptr_host, size_t bytes);
int xrs_host_free(void *ptr_host);
int xrs_memcpy_h2d(void *dst_dev, const void *src, size_t bytes, void *stream);
int xrs_memcpy_d2h(void *dst, const void *src_dev, size_t bytes, void *stream);
int xrs_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int xrs_memset(void *dst_dev, int byte_value, size_t bytes, void *stream);
/* Calibration: the streaming pattern of xrs_copy_f32 with ONE plane read and n_dst (1..8) planes written -- the ceiling
 * of a fused kernel's own read/write mix (HBM3E sustains less on write-heavy mixes than on a 1:1 copy).  `dsts_dev` is a
 * HOST array of device pointers.  Used by bench.py / tools/kbench.py next to xrs_copy_f32; not on the data path. */
int xrs_stream_mix_f32(const float *src_dev, float *const *dsts_dev, int n_dst, int64_t n, void *stream);
/* a rectangular window of a plane (pitches and width in bytes): `raster[top:bottom + 1, left:right + 1]` of a
 * device-resident raster (the slicing at the end of zonal.trim / zonal.crop, xrspatial/zonal.py:1841, 2058) */
int xrs_copy2d(void *dst_dev, size_t dst_pitch, const void *src_dev, size_t src_pitch, size_t width_bytes,
               int64_t rows, void *stream);
/* streaming plane copy in the library's own access pattern: the measured-copy-bandwidth calibration point */
/* `.astype(np.float32)` of the reference's wrappers (xrspatial/slope.py:82, hillshade.py:21, multispectral.py:834 ...)
 * on the device: numpy-backed rasters are sent in their own dtype and converted in HBM (round to nearest even). */
enum { XRS_DT_I8 = 0, XRS_DT_U8 = 1, XRS_DT_I16 = 2, XRS_DT_U16 = 3, XRS_DT_I32 = 4, XRS_DT_U32 = 5,
       XRS_DT_I64 = 6, XRS_DT_U64 = 7, XRS_DT_F64 = 8, XRS_DT_F32 = 9 };
int xrs_cast_f32(const void *src_dev, int src_dtype, float *dst_dev, int64_t n, void *stream);
int xrs_copy_f32(const float *src_dev, float *dst_dev, int64_t n, void *stream);
int xrs_stream_create(void **stream);
int xrs_stream_destroy(void *stream);
int xrs_stream_sync(void *stream);
int xrs_device_sync(void);
int xrs_event_create(void **event);
int xrs_event_destroy(void *event);
int xrs_event_record(void *event, void *stream);
int xrs_stream_wait_event(void *stream, void *event);   /* later work on `stream` waits for `event` (device side) */
int xrs_event_sync(void *event);
int xrs_event_elapsed_ms(void *start_event, void *stop_event, float *ms);

/* --------------------------------------------------------- 3x3 terrain family
 * One-cell NaN border on true raster edges.  Replace the runners
 *   slope      xrspatial/slope.py:79-83      (_run_numpy -> _cpu :56-76)
 *   aspect     xrspatial/aspect.py:56-90     (_run_numpy)
 *   curvature  xrspatial/curvature.py:44-49  (_run_numpy -> _cpu :31-41)
 *   hillshade  xrspatial/hillshade.py:20-35  (_run_numpy)
 * Arithmetic follows the reference's CPU path (float64 gradient sums), not its
 * all-float32 CuPy kernels.  Outputs are float32; hillshade can also write
 * float64 (out_f64 != 0), which is what the reference returns under NumPy >= 2. */
int xrs_slope_f32(const float *in_dev, float *out_dev, int64_t rows, int64_t cols,
                  int64_t ld_in, int64_t ld_out, double cellsize_x, double cellsize_y,
                  int halo_top, int halo_bot, void *stream);
int xrs_aspect_f32(const float *in_dev, float *out_dev, int64_t rows, int64_t cols,
                   int64_t ld_in, int64_t ld_out, int halo_top, int halo_bot, void *stream);
int xrs_curvature_f32(const float *in_dev, float *out_dev, int64_t rows, int64_t cols,
                      int64_t ld_in, int64_t ld_out, double cellsize,
                      int halo_top, int halo_bot, void *stream);
int xrs_hillshade_f32(const float *in_dev, void *out_dev, int out_f64, int64_t rows, int64_t cols,
                      int64_t ld_in, int64_t ld_out, double azimuth, double angle_altitude,
                      int halo_top, int halo_bot, void *stream);

/* Fused variant: one read of the DEM, up to four outputs.  Any of the output
 * pointers may be NULL (that product is skipped).  Same results as the four
 * separate calls.  (The reference's summarize_terrain, xrspatial/analytics.py,
 * makes three separate passes.) */
int xrs_terrain_fused_f32(const float *in_dev, float *slope_dev, float *aspect_dev,
                          float *curvature_dev, float *hillshade_dev,
                          int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                          double cellsize_x, double cellsize_y, double azimuth, double angle_altitude,
                          int halo_top, int halo_bot, void *stream);

/* Fused raster pass: ONE read of the raster, any subset of the four terrain products plus a focal mean
 * (focal.apply / focal_stats 'mean' with a 0/1 mask).  Replaces a sequence of separate reference passes over
 * the same DataArray -- hillshade (xrspatial/hillshade.py:20-35), slope (slope.py:56-76), aspect
 * (aspect.py:56-90), curvature (curvature.py:31-49), focal.apply with _calc_mean (focal.py:226-228, 305-326)
 * -- and returns bit-identical results to the separate entry points above / xrs_focal_stats_f32.
 * Any output pointer may be NULL.  3x3 and 5x5 masks on 16-byte-friendly rasters run as one kernel
 * (4 B read + 4 B written per product per cell); other shapes fall back to the separate launches
 * (`work_dev`: as for xrs_focal_stats_f32, may be NULL for masks up to 5x5).
 * Row shards: halo_top / halo_bot must be 0 (true raster edge) or >= max(1, krows/2). */
int xrs_raster_pass_f32(const float *in_dev, float *slope_dev, float *aspect_dev, float *curvature_dev,
                        float *hillshade_dev, float *focal_mean_dev, const double *kernel, int krows,
                        int kcols, void *work_dev, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                        double cellsize_x, double cellsize_y, double azimuth, double angle_altitude,
                        int halo_top, int halo_bot, void *stream);

/* The same pass over only the first and the last `edge_rows` rows of the raster (a row shard whose halo rows have just
 * arrived: the rows in between were launched earlier, while the exchange was in flight -- what a dask graph does with
 * map_overlap(depth, boundary=nan), slope.py:86-97, the scheduler does here with two streams).  ONE launch over two
 * segments of tile rows when the fused kernel takes the request (3x3 / 5x5 masks: results are those of xrs_raster_pass_f32
 * on the whole raster, bit for bit), the two sub-range calls otherwise (what any row split of that request gives).  The
 * one-launch form works in whole tile rows of 16 raster rows: besides the edges it also writes up to 15 rows BELOW the first
 * edge (rows [edge_rows, 16 * ceil(edge_rows / 16))) and up to 15 rows ABOVE the last one, with the values the whole-raster
 * pass gives them -- harmless on the stream that also runs the launch for the rows in between (same values), a write-write
 * race if that launch runs on another stream: keep both on one stream, or pass edge_rows % 16 == 0.  No other row between the
 * edges is written.  2 * edge_rows >= rows: the whole raster. */
int xrs_raster_pass_edges_f32(const float *in_dev, float *slope_dev, float *aspect_dev, float *curvature_dev,
                              float *hillshade_dev, float *focal_mean_dev, const double *kernel, int krows,
                              int kcols, void *work_dev, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                              double cellsize_x, double cellsize_y, double azimuth, double angle_altitude,
                              int halo_top, int halo_bot, int64_t edge_rows, void *stream);
/* For tests: what served the calling thread's LAST xrs_raster_pass_f32 / xrs_raster_pass_edges_f32 call, as text, items
 * joined by ';' in the order they were enqueued (a record of its own: xrs_debug_window_route is not touched).  A fused launch
 * is  pass(ops=<set>,K=<3|5>,nt=<0|1>,cmask=<0|1>,tiles=<across>x<down>,seg=<first segment's tile rows>+<tile rows skipped>)
 * with <set> the INSTANTIATED product set in the letters S, A, C, H ("-": the focal mean alone) -- slope alone reports SH --,
 * nt the non-temporal store variant, cmask a compile-time mask, and tiles the launched workgroups (256 columns x 16 rows).
 * The fall-backs are  terrain_fused(ops=<set>)  for the products the fused kernel leaves to xrs_terrain_fused_f32,
 * focal_stats(K=<rows>x<cols>)  for a focal mean handed to xrs_focal_stats_f32, and  edges_split(rows=<edge_rows>)  in front
 * of the items of the two sub-range calls the edges entry makes where one launch cannot take both edges.  Empty after a call
 * that launched nothing.  Returns the length of the text (as snprintf); at most buflen - 1 bytes and a NUL are written. */
int xrs_debug_pass_route(char *buf, size_t buflen);

/* Geodesic slope / aspect (method='geodesic'): WGS-84 ECEF -> local ENU plane fit per 3x3 window, float64
 * arithmetic, float32 out, NaN border, NaN if any of the nine elevations is NaN.  Replaces
 * _cpu_geodesic_slope / _cpu_geodesic_aspect (xrspatial/geodesic.py:181-229) behind slope.py:167-174 and
 * aspect.py:172-179.  elev_is_f64 selects the elevation element type (the reference widens to float64;
 * float32 rasters are widened in registers).  latlon_2d = 0: lat_dev[row] / lon_dev[col] are 1-D degree
 * coordinates (lat_dev points at the first OWNED row; halo rows' latitudes precede / follow it) and
 * `work_dev` must hold xrs_geodesic_workspace_bytes(rows + halo_top + halo_bot, cols) bytes for the
 * per-row / per-column trigonometry tables.  latlon_2d = 1: 2-D planes with pitch ld_latlon, no workspace.
 * aspect = 0 -> slope in degrees; 1 -> compass aspect, -1 where the fitted gradient is below 1e-7. */
size_t xrs_geodesic_workspace_bytes(int64_t rows_with_halos, int64_t cols);
int xrs_geodesic_f32(const void *elev_dev, int elev_is_f64, const double *lat_dev, const double *lon_dev,
                     int latlon_2d, float *out_dev, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                     int64_t ld_latlon, double a2, double b2, double z_factor, int aspect, void *work_dev,
                     int halo_top, int halo_bot, void *stream);

/* ----------------------------------------------------------- per-cell indices
 * Flat arrays of n float32 cells, NaN where the denominator is exactly 0.
 *   normalized_ratio  xrspatial/multispectral.py:825-841 (_normalized_ratio_cpu: ndvi/nbr/nbr2/ndmi)
 *   evi               xrspatial/multispectral.py:175-188 (_evi_cpu)
 *   savi              xrspatial/multispectral.py:876-890 (_savi_cpu) */
int xrs_normalized_ratio_f32(const float *a_dev, const float *b_dev, float *out_dev, int64_t n, void *stream);
int xrs_evi_f32(const float *nir_dev, const float *red_dev, const float *blue_dev, float *out_dev,
                int64_t n, double c1, double c2, double soil_factor, double gain, void *stream);
int xrs_savi_f32(const float *nir_dev, const float *red_dev, float *out_dev, int64_t n,
                 double soil_factor, void *stream);
/*   arvi  xrspatial/multispectral.py:29-43     gci   :350-361
 *   sipi  xrspatial/multispectral.py:1017-1031 ebbi  :1160-1174 */
int xrs_arvi_f32(const float *nir_dev, const float *red_dev, const float *blue_dev, float *out_dev,
                 int64_t n, void *stream);
int xrs_gci_f32(const float *nir_dev, const float *green_dev, float *out_dev, int64_t n, void *stream);
int xrs_sipi_f32(const float *nir_dev, const float *red_dev, const float *blue_dev, float *out_dev,
                 int64_t n, void *stream);
int xrs_ebbi_f32(const float *red_dev, const float *swir_dev, const float *tir_dev, float *out_dev,
                 int64_t n, void *stream);

/* ------------------------------------------------------------- k x k kernels
 * convolve2d: correlation with a float64 weight matrix given on the HOST
 * (krows x kcols, both odd, C order); NaN border of k//2 on true edges, NaNs
 * propagate.  Replaces _convolve_2d_numpy, xrspatial/convolution.py:285-313.
 * `work_dev` must hold xrs_kxk_workspace_bytes(krows, kcols) bytes (the weights
 * are staged there on `stream`). */
size_t xrs_kxk_workspace_bytes(int krows, int kcols);
int xrs_convolve2d_f32(const float *in_dev, float *out_dev, int64_t rows, int64_t cols,
                       int64_t ld_in, int64_t ld_out, const double *kernel, int krows, int kcols,
                       void *work_dev, int halo_top, int halo_bot, void *stream);

/* focal statistics over the window cells where kernel == 1 exactly, window clipped
 * to the raster (no NaN border), NaN cells skipped; all requested statistics in ONE
 * pass.  Replaces _apply_numpy with the built-in reducers, xrspatial/focal.py:305-326
 * and :268-302, i.e. focal.apply(func=_calc_*) and focal.focal_stats (:782-797).
 * stat_mask bit i selects XRS_STAT_*; outs_dev[i] (HOST array of 7 device
 * pointers) receives statistic i and may be NULL when its bit is clear. */
enum { XRS_STAT_MEAN = 0, XRS_STAT_MAX = 1, XRS_STAT_MIN = 2, XRS_STAT_RANGE = 3,
       XRS_STAT_STD = 4, XRS_STAT_VAR = 5, XRS_STAT_SUM = 6, XRS_NUM_STATS = 7 };
int xrs_focal_stats_f32(const float *in_dev, float *const *outs_dev, unsigned stat_mask,
                        int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                        const double *kernel, int krows, int kcols, void *work_dev,
                        int halo_top, int halo_bot, void *stream);
/* The same with accuracy options (xrs_focal_stats_f32 == flags 0).  Windows of 9x9 cells and more take float32 walkers
 * whose mean / var / std / sum agree with the reference's float64 accumulators to <= 2e-6 relative (a guard per output
 * sends ill-conditioned tiles to the exact kernels); the flags keep whole launches on the exact kernels instead:
 *   XRS_FOCAL_EXACT_MOMENTS   mean / var / std from float64 running sums (NaN-skipping, counted): ~1 ulp of the reference;
 *   XRS_FOCAL_SEQUENTIAL_SUM  `sum` added tap by tap in the reference's row-major order in float32 (numba's nansum keeps
 *                             the array dtype): bit-identical to the CPU path.
 * The host layer sets them from xrspatial_amd.focal.options / the XRS_FOCAL_SUM and XRS_FOCAL_MOMENTS variables. */
enum { XRS_FOCAL_EXACT_MOMENTS = 1, XRS_FOCAL_SEQUENTIAL_SUM = 2 };
int xrs_focal_stats_f32_ex(const float *in_dev, float *const *outs_dev, unsigned stat_mask,
                           int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                           const double *kernel, int krows, int kcols, void *work_dev, size_t work_bytes,
                           int halo_top, int halo_bot, unsigned flags, void *stream);
/* Device scratch xrs_focal_stats_f32_ex can use for a rows x cols raster: the float64 copy of the kernel
 * (xrs_kxk_workspace_bytes) plus one byte per tile for the separable box kernel -- np.ones((k, k)) masks, the ones the
 * reference's benchmark suite runs, get their variance / standard deviation (and the mean and sum beside them) from an
 * O(1)-per-cell walk that hands the tiles it cannot stand for (NaN / inf cells, flat windows) to the general kernel
 * through that map.  With a smaller workspace (or none) the general kernel runs everywhere: more time, and results that agree
 * with the separable walk's within the documented tolerance (float32 walker vs float64 column sums: ~2e-6 relative on var / std),
 * not bit for bit. */
size_t xrs_focal_workspace_bytes(int64_t rows, int64_t cols, int krows, int kcols);
/* For tests: which kernels served the calling thread's LAST xrs_focal_stats_f32 / xrs_focal_stats_f32_ex /
 * xrs_convolve2d_f32 call, as text, one item per launch group in launch order, joined by ';'.  An item is a walker's name
 * (focal_mom_circle, wide_annulus7, focal_ext_annulus_a, focal_box_f32, focal_mean_runs, boxsep ...) or a branch of the
 * dispatch (big, pass, strips3, strips5, lds_mean7, tap0 .. tap4, conv_strips3, conv_strips5, conv_tap) with (R) or
 * (R,RI), and for the strip walkers the tiling the launch chose: [wave=<wave-tile columns>,wg=<workgroup columns>,
 * rows=<tile rows>,grid=<workgroups across>x<down>].  Empty after a call that launched nothing.  Returns the length of
 * the text (as snprintf); at most buflen - 1 bytes and a NUL are written. */
int xrs_debug_window_route(char *buf, size_t buflen);

/* focal.apply with a user callable (func other than the built-in reducers): the kernel-shaped float32 arrays that
 * _apply_numpy, xrspatial/focal.py:305-326, builds per cell (NaN, then data[ky, kx] where kernel == 1 and inside the
 * raster), for the band of rows [y0, y0 + band_rows): windows_dev[band_rows][cols][krows][kcols].  The host calls the
 * callable on each.  in_dev is the whole raster (rows x cols, pitch ld_in); krows * kcols <= 2048. */
int xrs_focal_windows_f32(const float *in_dev, float *windows_dev, int64_t rows, int64_t cols, int64_t ld_in,
                          int64_t y0, int64_t band_rows, const double *kernel, int krows, int kcols, void *stream);

/* focal.mean: fixed 3x3 NaN-skipping mean on a clamped window, float64 out, cells
 * equal to one of `excludes` (NaN matches NaN) are passed through.  One pass;
 * the host loops `passes`.  Replaces _mean_numpy, xrspatial/focal.py:44-67.
 * in_is_f64 selects the input element type (first pass may read float32). */
int xrs_focal_mean3x3(const void *in_dev, int in_is_f64, double *out_dev, int64_t rows, int64_t cols,
                      int64_t ld_in, int64_t ld_out, const double *excludes, int n_excludes,
                      int halo_top, int halo_bot, void *stream);

/* `passes` applications in one call (the loop of focal.py:257-259): contiguous planes (pitch = cols), the passes
 * ping-pong between out_dev and scratch_dev (rows*cols doubles, may be NULL for passes == 1); result in out_dev. */
int xrs_focal_mean3x3_passes(const void *in_dev, int in_is_f64, double *out_dev, double *scratch_dev, int passes,
                             int64_t rows, int64_t cols, const double *excludes, int n_excludes, void *stream);

/* focal.hotspots support (xrspatial/focal.py:881-934): global NaN-skipping moments of a float32 plane
 * -> moments32_dev = { uint64 count; double sum, ssd (sum of squared deviations from the mean), mean },
 * and the z-score classifier  z = (mean_array - global_mean) / global_std  ->  {0, +-90, +-95, +-99} int8. */
int xrs_nan_moments_f32(const float *in_dev, int64_t n, void *moments32_dev, void *stream);
int xrs_hotspots_classify_f32(const float *mean_array_dev, signed char *out_dev, int64_t n,
                              float global_mean, float global_std, void *stream);

/* -------------------------------------------------------------------- classify
 * xrspatial.classify (reference: xrspatial/classify.py, CPU path).  Flat C-order rasters of n cells in their own dtype.
 *  bin:        _cpu_bin (:153-187): out = float32(new_values[b]) for the bin b of every cell, NaN where there is none.
 *              bins / new_values are float64 device arrays of n_bins; mode 0 = the reference's loop verbatim (any bins),
 *              1 = count of bins below the cell, 2 = bisection (1 and 2 only for non-decreasing, NaN-free bins).
 *  binary:     _cpu_binary (:31-41): 1 where the cell equals one of `values` (float64), else 0 (finite) / NaN (float).
 *  finite_stats: { count, min, max, sum } of the finite cells (float64; min / max NaN when there is none);
 *  sqdev:      { count, -, -, sum of (x - center)^2 } over the finite cells;  above: { count, -, -, sum } of finite x > threshold.
 *  select:     the ranks[i]-th smallest finite cells (0-based int64 ranks, ascending, < the finite count, <= 64 per call),
 *              as float64; MSB-first radix select over the order-preserving key.  n < 2^32.
 *  max_breaks: the unique finite values uv[0..M) (-0.0 == +0.0), their gaps in the input dtype and the n_top largest gaps
 *              by (gap, index) -> out = { M, (index, uv[index], uv[index + 1]) x n_top, uv[M-1], uv[0..n_top] }
 *              (NaN / -1 where there is none); n_top < 0: out = { M, uv[0..M) } (n + 1 doubles).  n < 2^31.
 * `work_dev` holds xrs_classify_workspace_bytes(n, values_f64) bytes (every entry point of this group fits in it). */
size_t xrs_classify_workspace_bytes(int64_t n, int values_f64);
int xrs_classify_to_f64(const void *in_dev, int dtype_code, double *out_dev, int64_t n, void *stream);
int xrs_classify_bin_f32(const float *in_dev, float *out_dev, int64_t n, const double *bins_dev,
                         const double *new_values_dev, int n_bins, int mode, void *stream);
int xrs_classify_bin_f64(const double *in_dev, float *out_dev, int64_t n, const double *bins_dev,
                         const double *new_values_dev, int n_bins, int mode, void *stream);
int xrs_classify_bin_i32(const int32_t *in_dev, float *out_dev, int64_t n, const double *bins_dev,
                         const double *new_values_dev, int n_bins, int mode, void *stream);
int xrs_classify_bin_i64(const int64_t *in_dev, float *out_dev, int64_t n, const double *bins_dev,
                         const double *new_values_dev, int n_bins, int mode, void *stream);
int xrs_classify_binary_f32(const float *in_dev, float *out_dev, int64_t n, const double *values_dev, int n_values, void *stream);
int xrs_classify_binary_f64(const double *in_dev, double *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_binary_i8(const int8_t *in_dev, int8_t *out_dev, int64_t n, const double *values_dev, int n_values,
                           void *stream);
int xrs_classify_binary_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n, const double *values_dev, int n_values,
                           void *stream);
int xrs_classify_binary_i16(const int16_t *in_dev, int16_t *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_binary_u16(const uint16_t *in_dev, uint16_t *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_binary_i32(const int32_t *in_dev, int32_t *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_binary_u32(const uint32_t *in_dev, uint32_t *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_binary_i64(const int64_t *in_dev, int64_t *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_binary_u64(const uint64_t *in_dev, uint64_t *out_dev, int64_t n, const double *values_dev, int n_values,
                            void *stream);
int xrs_classify_finite_stats_f32(const float *in_dev, int64_t n, void *work_dev, double *out4_dev, void *stream);
int xrs_classify_finite_stats_f64(const double *in_dev, int64_t n, void *work_dev, double *out4_dev, void *stream);
int xrs_classify_sqdev_f32(const float *in_dev, int64_t n, double center, void *work_dev, double *out4_dev, void *stream);
int xrs_classify_sqdev_f64(const double *in_dev, int64_t n, double center, void *work_dev, double *out4_dev, void *stream);
int xrs_classify_above_f32(const float *in_dev, int64_t n, double threshold, void *work_dev, double *out4_dev, void *stream);
int xrs_classify_above_f64(const double *in_dev, int64_t n, double threshold, void *work_dev, double *out4_dev, void *stream);
int xrs_classify_select_f32(const float *in_dev, int64_t n, const int64_t *ranks_dev, int n_ranks, void *work_dev,
                            size_t work_bytes, double *values_dev, void *stream);
int xrs_classify_select_f64(const double *in_dev, int64_t n, const int64_t *ranks_dev, int n_ranks, void *work_dev,
                            size_t work_bytes, double *values_dev, void *stream);
int xrs_classify_max_breaks_f32(const float *in_dev, int64_t n, int n_top, void *work_dev, size_t work_bytes,
                                double *out_dev, void *stream);
int xrs_classify_max_breaks_f64(const double *in_dev, int64_t n, int n_top, void *work_dev, size_t work_bytes,
                                double *out_dev, void *stream);

/* -------------------------------------------------------------------- zonal
 * Per-zone partial reductions of one streaming pass over (zone index, value):
 * count (integer-exact), sum and sum of squares (float64), min, max.  Cells with
 * zone index < 0 or >= n_zones, non-finite values, and values == nodata (when
 * has_nodata) are skipped.  The five output arrays (n_zones entries each) are
 * ACCUMULATED into: initialise them with xrs_zonal_init().  sum / sumsq hold the sums of
 * (x - shift) and (x - shift)^2 for the caller's `shift` (any value near the data: mean = shift + sum / n,
 * var = (sumsq - sum^2 / n) / n then stays well conditioned for rasters with a large offset and a small
 * spread; 0 gives the plain sums).  These partials are
 * the per-block statistics of the reference's dask path (_DASK_BLOCK_STATS,
 * xrspatial/zonal.py:83-89) from which mean/std/var follow (:100-102); the
 * NumPy path they replace is _stats_numpy (:280-332). */
int xrs_zonal_init(uint64_t *count_dev, double *sum_dev, double *sumsq_dev,
                   float *min_dev, float *max_dev, int n_zones, void *stream);
int xrs_zonal_partials_f32(const int32_t *zone_idx_dev, const float *values_dev, int64_t n,
                           int n_zones, float nodata, int has_nodata, double shift,
                           uint64_t *count_dev, double *sum_dev, double *sumsq_dev,
                           float *min_dev, float *max_dev, void *stream);
/* Same reduction straight from the RAW int32 zone raster: `lut_dev[id - zone_min]` (zone_range entries, built from
 * xrs_zonal_scan / xrs_zonal_presence) gives the dense index of an id, -1 for ids that are not a zone; ids outside the
 * window belong to no zone.  Saves materialising the dense index raster (4 B written + 4 B read per cell) when only
 * the partial-sum statistics are wanted (np.unique(zones) + per-zone masks in the reference, zonal.py:290-311). */
int xrs_zonal_partials_lut_f32(const int32_t *zones_dev, int32_t zone_min, int32_t zone_range, const int32_t *lut_dev,
                               const float *values_dev, int64_t n, int n_zones, float nodata, int has_nodata, double shift,
                               uint64_t *count_dev, double *sum_dev, double *sumsq_dev, float *min_dev, float *max_dev,
                               void *stream);
int xrs_zonal_partials_lut_f64(const int32_t *zones_dev, int32_t zone_min, int32_t zone_range, const int32_t *lut_dev,
                               const double *values_dev, int64_t n, int n_zones, double nodata, int has_nodata, double shift,
                               uint64_t *count_dev, double *sum_dev, double *sumsq_dev, double *min_dev, double *max_dev,
                               void *stream);
/* ONE pass from the raw int32 zone raster WITHOUT a discovery pass in front (np.unique(zones) of zonal.py:290 folded into the
 * reduction): the caller GUESSES a window of ids [zone_base, zone_base + window) -- xrs_zonal_sample_* below reads a strided
 * sample of the rasters for that -- and the kernel accumulates straight into window-indexed tables (entry id - zone_base;
 * window <= 5000 ids: the tables live in LDS), which it initialises itself (overwritten, not accumulated into).
 * present_dev[id - zone_base] = 1 (window bytes) for ids that occur with invalid values only (count 0: the reference still
 * lists such a zone); *overflow_dev = 1 if some cell's id lies outside the window -- the tables are then incomplete and the
 * caller takes the two-pass route (xrs_zonal_scan_presence_i32 + xrs_zonal_partials_lut_*). */
int xrs_zonal_partials_window_f32(const int32_t *zones_dev, int32_t zone_base, int window, const float *values_dev, int64_t n,
                                  float nodata, int has_nodata, double shift, uint64_t *count_dev, double *sum_dev,
                                  double *sumsq_dev, float *min_dev, float *max_dev, unsigned char *present_dev,
                                  int32_t *overflow_dev, void *stream);
int xrs_zonal_partials_window_f64(const int32_t *zones_dev, int32_t zone_base, int window, const double *values_dev, int64_t n,
                                  double nodata, int has_nodata, double shift, uint64_t *count_dev, double *sum_dev,
                                  double *sumsq_dev, double *min_dev, double *max_dev, unsigned char *present_dev,
                                  int32_t *overflow_dev, void *stream);
/* n_samples cells at an odd stride through both rasters -> result24_dev = { int32 zmin, zmax; double SUM of the valid
 * values; uint64 number of valid values }: the id window to guess and (sum / count) a shift for the moments, from two tiny
 * launches. */
int xrs_zonal_sample_f32(const int32_t *zones_dev, const float *values_dev, int64_t n, int64_t n_samples, float nodata,
                         int has_nodata, void *result24_dev, void *stream);
int xrs_zonal_sample_f64(const int32_t *zones_dev, const double *values_dev, int64_t n, int64_t n_samples, double nodata,
                         int has_nodata, void *result24_dev, void *stream);
/* float64 values (the reference does not cast `values`: float64 and integer rasters keep
 * their precision; integers are widened to float64 by the host layer).  min/max are float64. */
int xrs_zonal_init_f64(uint64_t *count_dev, double *sum_dev, double *sumsq_dev,
                       double *min_dev, double *max_dev, int n_zones, void *stream);
int xrs_zonal_partials_f64(const int32_t *zone_idx_dev, const double *values_dev, int64_t n,
                           int n_zones, double nodata, int has_nodata, double shift,
                           uint64_t *count_dev, double *sum_dev, double *sumsq_dev,
                           double *min_dev, double *max_dev, void *stream);

/* Dense zone indexing on the device (replaces the host-side np.unique of xrspatial/zonal.py:290 for
 * integral zone ids): zone_dtype 0 = int32, 1 = int64, 2 = float32, 3 = float64.
 *   xrs_zonal_scan      -> result32_dev = { double zmin, zmax; uint64 n_finite; int32 all_integral, pad }
 *   xrs_zonal_presence  -> present_dev[id - zmin] = 1 for every finite id in [zmin, zmin + range)
 *   xrs_zonal_index     -> idx_dev[cell] = lut_dev[id - zmin], -1 for non-finite / out-of-range ids */
int xrs_zonal_scan(const void *zones_dev, int zone_dtype, int64_t n, void *result32_dev, void *stream);
/* scan + presence in ONE read for int32 ids: ids inside the optimistic window [0, window) are marked in present_dev
 * (window bytes) during the scan; if the scan result shows 0 <= zmin and zmax < window the map is complete and
 * xrs_zonal_presence is not needed. */
int xrs_zonal_scan_presence_i32(const int32_t *zones_dev, int64_t n, void *result32_dev, unsigned char *present_dev,
                                int window, void *stream);
int xrs_zonal_presence(const void *zones_dev, int zone_dtype, int64_t n, double zmin, int64_t range,
                       unsigned char *present_dev, void *stream);
int xrs_zonal_index(const void *zones_dev, int zone_dtype, int64_t n, double zmin, int64_t range,
                    const int32_t *lut_dev, int32_t *idx_dev, void *stream);

/* zonal.crosstab, 2-D values (xrspatial/zonal.py:699-800): counts_dev[zone * n_cats + cat] += number of cells
 * with that (dense zone index, dense category index) pair; negative / out-of-range indices are skipped.
 * counts_dev (n_zones * n_cats uint64) is accumulated into: zero it with xrs_memset first. */
int xrs_crosstab_counts(const int32_t *zone_idx_dev, const int32_t *cat_idx_dev, int64_t n, int n_zones,
                        int n_cats, uint64_t *counts_dev, void *stream);

/* majority (most frequent valid value per zone, ties -> smallest; NaN for zones without a valid
 * cell), computed by two device radix sorts + run voting; replaces _stats_majority applied per zone
 * (xrspatial/zonal.py:56-68, 144-163).  `work_dev` must hold
 * xrs_zonal_majority_workspace_bytes(n, n_zones, values_f64) bytes.  n < 2^31 cells per call. */
size_t xrs_zonal_majority_workspace_bytes(int64_t n, int n_zones, int values_f64);
int xrs_zonal_majority_f32(const int32_t *zone_idx_dev, const float *values_dev, int64_t n, int n_zones,
                           float nodata, int has_nodata, void *work_dev, size_t work_bytes,
                           double *majority_dev, void *stream);
int xrs_zonal_majority_f64(const int32_t *zone_idx_dev, const double *values_dev, int64_t n, int n_zones,
                           double nodata, int has_nodata, void *work_dev, size_t work_bytes,
                           double *majority_dev, void *stream);
/* majority WITHOUT a sort (csrc/zonal_mode.hip): the cells are routed zone by zone and then, inside a zone, by a hash
 * of the value's bits until every part fits an LDS hash table that counts multiplicities; same result as
 * xrs_zonal_majority_* (ties -> smallest value, -0.0 == +0.0, NaN for a zone without a valid cell) at ~1/6 of the traffic.
 * majority_dev holds n_zones + 1 doubles: the LAST one counts the threads that could not place a key because the table of
 * their part was full -- nonzero means the results are not valid and the caller must use xrs_zonal_majority_*.  That
 * depends on the DISTINCT values of a part, not on the size of the zone: a part overflows when more than 2048 of its
 * distinct values share their slot of the count-only table with another cell.  Spread by the hash, that takes a zone of
 * more than ~2^27 cells of all-distinct values; a few thousand values chosen to hash to one part do it in a zone of 6000
 * cells.  n_zones <= xrs_zonal_mode_max_zones(); n < 2^31; `work_dev` holds
 * xrs_zonal_mode_workspace_bytes(n, n_zones, values_f64) bytes and begins, after the call, with five uint32 that describe
 * the plan it ran: n_valid (valid cells), n_parts (sum over the zones of their 2^B parts), n_chunks (8192-key chunks of
 * the zones cut into parts), overflow (the count above) and n_direct (zones of more than 2^11 parts).  zone_counts_dev: the valid cells per zone as uint32 if the
 * caller has them (the `count` of xrs_zonal_partials_* for the same rasters and nodata value), else NULL -- they are
 * then counted here with one more pass over the rasters. */
size_t xrs_zonal_mode_workspace_bytes(int64_t n, int n_zones, int values_f64);
int xrs_zonal_mode_max_zones(void);
int xrs_zonal_mode_f32(const int32_t *zone_idx_dev, const float *values_dev, int64_t n, int n_zones, float nodata,
                       int has_nodata, const uint32_t *zone_counts_dev, void *work_dev, size_t work_bytes, double *majority_dev,
                       void *stream);
int xrs_zonal_mode_f64(const int32_t *zone_idx_dev, const double *values_dev, int64_t n, int n_zones, double nodata,
                       int has_nodata, const uint32_t *zone_counts_dev, void *work_dev, size_t work_bytes, double *majority_dev,
                       void *stream);
/* the valid cells of every zone gathered into one contiguous run, for statistics that are arbitrary host callables
 * (zonal.stats(stats_funcs={name: callable}): _calc_stats, xrspatial/zonal.py:144-163, slices the argsort-ordered
 * values per zone and filters non-finite / nodata cells before calling func).  sorted_values_dev[n] receives the cells
 * ordered by (zone index, value ascending); cells outside [0, n_zones) or with an invalid value come last (as NaN), so
 * zone z's values are the slice [sum(count[:z]), sum(count[:z+1])) with count from xrs_zonal_partials_*.  Workspace:
 * xrs_zonal_majority_workspace_bytes(n, n_zones, values_f64).  n < 2^31 cells per call. */
int xrs_zonal_group_f32(const int32_t *zone_idx_dev, const float *values_dev, int64_t n, int n_zones, float nodata,
                        int has_nodata, void *work_dev, size_t work_bytes, float *sorted_values_dev, void *stream);
int xrs_zonal_group_f64(const int32_t *zone_idx_dev, const double *values_dev, int64_t n, int n_zones, double nodata,
                        int has_nodata, void *work_dev, size_t work_bytes, double *sorted_values_dev, void *stream);

/* return_type='xarray.DataArray' of zonal.stats (xrspatial/zonal.py:313-332): out[s][cell] =
 * table[s][zone_idx[cell]] (row-major n_stats x n_zones float64 table), NaN where the cell has no zone. */
int xrs_zonal_backproject_f64(const int32_t *zone_idx_dev, int64_t n, const double *table_dev, int n_stats,
                              int n_zones, double *out_dev, void *stream);

/* zonal.trim / zonal.crop (xrspatial/zonal.py:1651-1731 `_trim`, :1845-1940 `_crop`): bounding box of the cells
 * that equal one of `values` (host array, at most 16; invert = 0: crop's zone ids) or equal none of them
 * (invert = 1: trim's nodata values).  Cells are compared as float64, NaN equals nothing (`e == val` upstream).
 * box4_dev = { top, bottom, left, right }; { rows, -1, cols, -1 } when no cell qualifies.  `dtype`: XRS_DT_*. */
int xrs_match_bbox(const void *data_dev, int dtype, int64_t rows, int64_t cols, int64_t ld, const double *values,
                   int n_values, int invert, int *box4_dev, void *stream);

/* zonal.regions (xrspatial/zonal.py:1406-1549 `_area_connectivity`, :1552-1636 `regions`): connected-region labels of a
 * rows x cols C-contiguous raster (`dtype`: XRS_DT_*; at most 2^32 - 1 cells), 4- or 8-connected, with the reference's
 * clamped windows and its tolerance abs_T(w - v) <= 1e-08 + 1e-05 * abs_T(v).  Two calls on one caller-owned
 * workspace of xrs_regions_workspace_bytes(rows, cols) bytes, same raster and neighborhood:
 *   xrs_regions_link:  links within tiles and counts the cells that open a new region; *n_new (host) receives the count,
 *                      which is the largest label (the call waits for the stream);
 *   xrs_regions_label: merges across tile borders and writes every cell's label into out_dev (same dtype; NaN kept). */
size_t xrs_regions_workspace_bytes(int64_t rows, int64_t cols);
int xrs_regions_link(const void *data_dev, int dtype, int64_t rows, int64_t cols, int neighborhood, void *work_dev,
                     uint64_t *n_new, void *stream);
int xrs_regions_label(const void *data_dev, int dtype, int64_t rows, int64_t cols, int neighborhood, void *work_dev,
                      void *out_dev, void *stream);

/* perlin / generate_terrain (xrspatial/perlin.py:51-91 `_perlin`, `_perlin_numpy` and the 16 launches of `_perlin_cupy` /
 * `_terrain_gpu`, :129-186 and terrain.py:130-180; terrain.py:36-80 `_gen_terrain`, `_terrain_numpy`): lattice noise with the
 * NumPy path's typing.
 *   xrs_noise_raw_*: ONE launch writes rows [row0, row0 + rows) of a total_rows x cols raster into out_dev (rows x cols,
 *     C-contiguous) -- a banded or sharded plane is bit-identical to the whole one -- and leaves { min, max } of what it
 *     wrote in minmax_dev[0..1] ({ +inf, -inf } for an empty call).  Coordinates are
 *     np.linspace(x0, x1, cols, endpoint=False, dtype=float32) by np.linspace(y0, y1, total_rows, ...).  `tables`: HOST
 *     array of n_octaves device pointers, table i = RandomState(seed + i).permutation(2^20) as int32 (not doubled).
 *     mode 0 (perlin, n_octaves == 1): the noise stored in the output dtype (perlin.py:89).  mode 1 (terrain, up to 16
 *     octaves): h = T(h + noise_i / 2^i) per octave, h / T(1.97), h ** 3 (terrain.py:50-60).  Every lattice index has to stay
 *     in [0, 2^20 - 1); a range that does not is refused.
 *   xrs_noise_finish_*: in place, (v - min) / (max - min) in the plane's dtype (perlin.py:90, terrain.py:76), then
 *     v < threshold -> 0 (terrain.py:77) and v * scale (terrain.py:78) where asked for.  min / max pass through the host
 *     between the two calls: a sharded caller reduces them across ranks there. */
int xrs_noise_raw_f32(float *out_dev, int64_t rows, int64_t cols, int64_t row0, int64_t total_rows, double x0, double x1,
                      double y0, double y1, const int32_t *const *tables, int n_octaves, int mode, double *minmax_dev,
                      void *stream);
int xrs_noise_raw_f64(double *out_dev, int64_t rows, int64_t cols, int64_t row0, int64_t total_rows, double x0, double x1,
                      double y0, double y1, const int32_t *const *tables, int n_octaves, int mode, double *minmax_dev,
                      void *stream);
int xrs_noise_finish_f32(float *data_dev, int64_t n, double min, double max, int has_threshold, double threshold,
                         int has_scale, double scale, void *stream);
int xrs_noise_finish_f64(double *data_dev, int64_t n, double min, double max, int has_threshold, double threshold,
                         int has_scale, double scale, void *stream);

/* viewshed (xrspatial/viewshed.py, the CPU sweep `_viewshed_cpu` / `_viewshed_cpu_sweep`): which cells of a rows x cols
 * C-contiguous raster (both at least 2) are seen from cell (view_row, view_col), as a per-cell predicate that equals the
 * sweep's result.  All arithmetic is float64 whatever the raster's dtype; the viewpoint's elevation is
 * data[view_row, view_col] + observer_elev, read on the device.  ew_res / ns_res: the coordinate steps along x / y (only
 * their squares matter).  out_dev (float64): 180 at the viewpoint, -1 where invisible, else the vertical angle in degrees
 * (`_get_vertical_ang`).  NaN cells are never visible and never hide a cell.  Two launches on the stream: the three event
 * gradients of every cell into work_dev (xrs_viewshed_workspace_bytes(rows, cols) bytes, caller-owned), then one ray walk
 * per cell. */
size_t xrs_viewshed_workspace_bytes(int64_t rows, int64_t cols);
int xrs_viewshed_f32(const float *data_dev, int64_t rows, int64_t cols, int64_t view_row, int64_t view_col, double observer_elev,
                     double target_elev, double ew_res, double ns_res, void *work_dev, double *out_dev, void *stream);
int xrs_viewshed_f64(const double *data_dev, int64_t rows, int64_t cols, int64_t view_row, int64_t view_col, double observer_elev,
                     double target_elev, double ew_res, double ns_res, void *work_dev, double *out_dev, void *stream);

/* hillshade(shadows=True) (xrspatial/gpu_rtx/hillshade.py `_hillshade_rt` and gpu_rtx/mesh_utils.py `create_triangulation`,
 * which trace the raster's triangle mesh through OptiX): replaced by one ray walk per cell over the same mesh, the result
 * stated as a rule in DESIGN.md §6i and evaluated in float64.  data_dev: rows x cols C-contiguous, every cell finite (the caller
 * checks).  scale: the reference's max(rows, cols) / max of the raster; zmin / zmax: bounds of the raster's values (the walk
 * stops where a ray is above zmax * scale or below zmin * scale for good).  sun_*: the unit vector towards the sun, x along
 * the columns, y along the rows.  shadows = 0 leaves the shadow rays out: Lambert's shade on the mesh's normals alone.
 * out_dev (float32): the shade in [0, 1], halved where the cell's shadow ray hits the mesh; NaN on the border rows and columns.
 * Two launches on the stream: the float32 vertex heights and a table of block maxima into work_dev
 * (xrs_hillshade_shadow_workspace_bytes(rows, cols) bytes, caller-owned), then the walk.
 * The probe entry points are for measuring (tools/hillshade_shadow_bench.py): the same walk with the block level over
 * `block` x `block` cells (8, 16, 32; 0 = none; the entry points above use 32) and, where counts4_dev is not null, the
 * { sum, max } of cells visited and { sum, max } of blocks tested per ray added into its four zeroed uint64. */
size_t xrs_hillshade_shadow_workspace_bytes(int64_t rows, int64_t cols);
int xrs_hillshade_shadow_f32(const float *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax, double sun_x,
                             double sun_y, double sun_z, int shadows, void *work_dev, float *out_dev, void *stream);
int xrs_hillshade_shadow_f64(const double *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax, double sun_x,
                             double sun_y, double sun_z, int shadows, void *work_dev, float *out_dev, void *stream);
int xrs_hillshade_shadow_probe_f32(const float *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,
                                   double sun_x, double sun_y, double sun_z, int block, void *work_dev, float *out_dev,
                                   uint64_t *counts4_dev, void *stream);
int xrs_hillshade_shadow_probe_f64(const double *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,
                                   double sun_x, double sun_y, double sun_z, int block, void *work_dev, float *out_dev,
                                   uint64_t *counts4_dev, void *stream);

/* viewshed(method='mesh') (xrspatial/gpu_rtx/viewshed.py `_viewshed_rt` and gpu_rtx/mesh_utils.py `create_triangulation`, which
 * trace one ray per cell through OptiX from the cell's surface point on the raster's triangle mesh to the observer): replaced by
 * one bounded ray walk per cell over the same mesh, the result stated as a rule in DESIGN.md §6l and evaluated in float64.
 * data_dev: rows x cols C-contiguous, at least 2 x 2, every cell finite (the caller checks).  scale, zmin, zmax: as for
 * xrs_hillshade_shadow_*.  view_row / view_col: the observer's cell.  observer_elev / target_elev: heights in the raster's own
 * units (scaled for the rays here, unscaled for the angles); ew_res / ns_res: the cell sizes that enter the angles only.
 * out_dev (float32): 180 at the viewpoint, -1 where the cell's sight line hits the mesh, else the vertical angle in degrees.
 * Two launches on the stream: the float32 vertex heights and a table of block maxima into work_dev
 * (xrs_viewshed_mesh_workspace_bytes(rows, cols) bytes, caller-owned; the layout of xrs_hillshade_shadow_workspace_bytes),
 * then the walk.  The probe entry points are for measuring (tools/viewshed_mesh_bench.py): the same walk with the block level
 * over `block` x `block` cells (8, 16, 32; 0 = none; the entry points above use 32) and, where counts4_dev is not null, the
 * { sum, max } of cells visited and { sum, max } of blocks tested per ray added into its four zeroed uint64. */
size_t xrs_viewshed_mesh_workspace_bytes(int64_t rows, int64_t cols);
int xrs_viewshed_mesh_f32(const float *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax, int64_t view_row,
                          int64_t view_col, double observer_elev, double target_elev, double ew_res, double ns_res, void *work_dev,
                          float *out_dev, void *stream);
int xrs_viewshed_mesh_f64(const double *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax, int64_t view_row,
                          int64_t view_col, double observer_elev, double target_elev, double ew_res, double ns_res, void *work_dev,
                          float *out_dev, void *stream);
int xrs_viewshed_mesh_probe_f32(const float *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,
                                int64_t view_row, int64_t view_col, double observer_elev, double target_elev, double ew_res,
                                double ns_res, int block, void *work_dev, float *out_dev, uint64_t *counts4_dev, void *stream);
int xrs_viewshed_mesh_probe_f64(const double *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,
                                int64_t view_row, int64_t view_col, double observer_elev, double target_elev, double ew_res,
                                double ns_res, int block, void *work_dev, float *out_dev, uint64_t *counts4_dev, void *stream);

/* proximity / allocation / direction (xrspatial/proximity.py `_process`): for every cell of a rows x cols C-contiguous raster
 * (`dtype`: XRS_DT_*) the exact nearest target, with the reference's float64 distance arithmetic rounded to float32, the
 * sweep's order among equidistant targets and its max_distance cut.
 *   targets    n_values == 0: cells that are non-zero and finite; else cells equal to one of the n_values 8-byte values at
 *              values_dev, read as `values_kind` says: float64 (every cell compared as float64, NumPy's promotion), or int64 /
 *              uint64 for integer rasters (compared as integers: values beyond 2^53 stay apart).
 *   xs_dev / ys_dev: one float64 coordinate per column / row, finite and strictly monotonic (the caller checks).
 *   gc_dev     GREAT_CIRCLE only (else may be null): np.radians(xs) (cols), np.radians(ys) (rows), np.cos(np.radians(ys))
 *              (rows), one after the other.
 *   metric     0 EUCLIDEAN, 1 GREAT_CIRCLE, 2 MANHATTAN (the reference's codes).
 *   mode       0 proximity, 1 allocation, 2 direction: one float32 plane of rows * cols into out_dev; 3: all three planes, in
 *              that order, 3 * rows * cols floats, each bit-equal to what modes 0, 1, 2 write.
 *              | XRS_PROX_SCAN_ONLY: only the row scan into work_dev; max_distance, metric and the product bits are not
 *              read, out_dev is not written and may be null.  | XRS_PROX_SEARCH_ONLY: only the search, on a workspace that
 *              holds the same raster's scan; work_dev is read only, out_dev must not be null.  Both bits at once, or any bit
 *              beside these two and the product, are refused.
 *   work_dev   xrs_proximity_workspace_bytes(rows, cols) bytes, caller-owned.  Its layout is part of the ABI (SEARCH_ONLY
 *              consumes it); with up256(n) = n rounded up to a multiple of 256, byte offsets from work_dev:
 *                left   0                                    int32[rows * cols]  largest target column <= j of the row, -1: none
 *                right  up256(4 rows cols)                   int32[rows * cols]  smallest target column > j, -1: none
 *                flag   2 up256(4 rows cols)                 int32[rows]         1 where the row holds a target, else 0
 *                list   flag + up256(4 rows)                 int32[rows]         the rows with a target, ascending; only the
 *                                                                                first `count` entries are written
 *                count  list + up256(4 rows)                 int32[1]            their number
 *              and the size is count + 256.  Nothing outside these arrays is written.
 * Ties: of several targets at the smallest float32 distance those in rows <= i come first, there the first in row-major
 * order, among rows > i the last.  EUCLIDEAN and MANHATTAN follow that at every cell, runs of equidistant targets inside one
 * row (long thin cells, distances that underflow) included; GREAT_CIRCLE names the nearest of such a run on either side.
 * Three launches on the stream (scan, row list, search); cells without a target within max_distance are NaN. */
enum { XRS_PROX_VALUES_F64 = 0, XRS_PROX_VALUES_I64 = 1, XRS_PROX_VALUES_U64 = 2 };
enum { XRS_PROX_SCAN_ONLY = 16, XRS_PROX_SEARCH_ONLY = 32 };
size_t xrs_proximity_workspace_bytes(int64_t rows, int64_t cols);
int xrs_proximity(const void *data_dev, int dtype, int64_t rows, int64_t cols, const double *xs_dev, const double *ys_dev,
                  const double *gc_dev, const void *values_dev, int values_kind, int n_values, double max_distance, int metric,
                  int mode, void *work_dev, float *out_dev, void *stream);

/* a_star_search (xrspatial/pathfinding.py:145-230 `_a_star_search`, :86-106 `_find_nearest_pixel`, :233-382 `a_star_search`): the
 * shortest 4- or 8-connected path from (start_row, start_col) to (goal_row, goal_col) over the crossable cells of a rows x cols
 * C-contiguous raster (`dtype`: XRS_DT_*; at most XRS_ASTAR_MAX_CELLS cells), as the exact shortest-distance field from the goal
 * and one walk along it from the start.  Steps cost 1.0 along rows and columns and sqrt(2) diagonally.
 *   crossable  not NaN and equal to none of the n_barriers 8-byte values at barriers_dev, read as `barriers_kind` says
 *              (XRS_PROX_VALUES_*, as xrs_proximity reads its target values).
 *   snap_flags XRS_ASTAR_SNAP_START / XRS_ASTAR_SNAP_GOAL: a start / goal that is not crossable moves to the crossable cell at
 *              the smallest squared pixel distance, the first in row-major order among equals, strictly nearer than the raster's
 *              diagonal; to (-1, -1) when there is none.  XRS_ASTAR_NO_WALK: the field only, out_dev stays NaN.  Bits 8 .. 15:
 *              relaxation passes per host round trip, 1 .. 64 (0: the default).
 *   work_dev   xrs_astar_workspace_bytes(rows, cols) bytes, caller-owned (0 for an empty or too large raster).
 *   out_dev    float64: 0.0 at the start, the running sum of the step costs in walk order at every further cell of the path,
 *              NaN everywhere else; all NaN when there is no path.
 *   status_host HOST array of 8 words: start row, start col, goal row, goal col after snapping (-1, -1: none); flags; a and b,
 *              the path's numbers of straight and diagonal steps (-1 without a path); relaxation passes run.  Flags:
 *              XRS_ASTAR_START_CROSSABLE / XRS_ASTAR_GOAL_CROSSABLE tell of the cell the reference's warning looks at, which
 *              for (-1, -1) is the raster's last cell; XRS_ASTAR_PATH_FOUND.
 * The call waits for the stream (once per group of passes).  At most rows * cols + 2 passes; beyond that it fails.
 * xrs_astar_tile_visits: how many tiles (64 x 32 cells; each loads 66 x 34 words of the field) the passes of the last xrs_astar
 * call on this workspace worked on, summed over the passes -- what tools/pathfinding_bench.py turns into bytes per pass. */
enum { XRS_ASTAR_SNAP_START = 1, XRS_ASTAR_SNAP_GOAL = 2, XRS_ASTAR_NO_WALK = 4, XRS_ASTAR_GROUP_SHIFT = 8 };
enum { XRS_ASTAR_START_CROSSABLE = 1, XRS_ASTAR_GOAL_CROSSABLE = 2, XRS_ASTAR_PATH_FOUND = 4 };
enum { XRS_ASTAR_MAX_CELLS = 1 << 30 };
size_t xrs_astar_workspace_bytes(int64_t rows, int64_t cols);
int xrs_astar(const void *data_dev, int dtype, int64_t rows, int64_t cols, int64_t start_row, int64_t start_col, int64_t goal_row,
              int64_t goal_col, const void *barriers_dev, int barriers_kind, int n_barriers, int connectivity, int snap_flags,
              void *work_dev, double *out_dev, int64_t *status_host, void *stream);
int xrs_astar_tile_visits(const void *work_dev, int64_t rows, int64_t cols, int64_t *visits_host, void *stream);

/* polygonize (xrspatial/experimental/polygonize.py:247-345 `_calculate_regions`, :105-207 `_follow`, :406-448 `_scan`): the
 * polygon rings of the connected regions of a rows x cols C-contiguous raster (`dtype`: XRS_DT_*; at most 2^32 - 1 cells), 4- or
 * 8-connected, in the reference's polygon order, ring order, start vertex and vertex sequence (the closed form: DESIGN.md §6h).
 * Three calls on one stream, same raster and shape; the first two wait for the stream (once, and once per group of rounds):
 *   xrs_polygonize_census   mask_dev: NULL or a plane of `mask_dtype` (XRS_DT_*; bool as XRS_DT_U8), a cell counts where it is
 *              != 0.  work_dev: xrs_polygonize_workspace_bytes(rows, cols) bytes, caller-owned; its first rows * cols uint32
 *              words are the region plane afterwards (0 = masked, else 1 + the number of regions whose first cell comes earlier).
 *              *n_regions, *n_states (host): the number of regions and of boundary states (cell, direction E / N / W / S, with
 *              the cell on the right-hand side outside the region).  No further call is needed when *n_states is 0.
 *   xrs_polygonize_rings    rings_dev: xrs_polygonize_rings_workspace_bytes(n_states) bytes, caller-owned (0 when n_states is 0 or
 *              above XRS_POLYGONIZE_MAX_STATES).  *n_rings, *n_points (host): the number of rings, and of points with every
 *              ring's closing point.  rounds (host, 2 words or NULL): the pointer-doubling rounds run to find every ring's start
 *              and to rank its states; each is bounded by 32, beyond which the call fails.
 *   xrs_polygonize_scatter  transform_host: NULL or 6 doubles, x = t0 * i + t1 * j + t2, y = t3 * i + t4 * j + t5 with separately
 *              rounded products and sums.  points_dev: float64 [n_points][2]; ring_offsets_dev: int64 [n_rings + 1], ring k
 *              owns points ring_offsets[k] .. ring_offsets[k + 1]; polygon_offsets_dev: int64 [n_regions + 1], polygon p (region
 *              p + 1) owns rings polygon_offsets[p] .. polygon_offsets[p + 1], the exterior first, then the holes by start cell;
 *              column_dev: [n_regions] values of the raster's dtype, each region's first cell.  Does not wait for the stream. */
#define XRS_POLYGONIZE_MAX_STATES 2147483647ull
size_t xrs_polygonize_workspace_bytes(int64_t rows, int64_t cols);
size_t xrs_polygonize_rings_workspace_bytes(uint64_t n_states);
int xrs_polygonize_census(const void *data_dev, int dtype, const void *mask_dev, int mask_dtype, int64_t rows, int64_t cols,
                          int connectivity, void *work_dev, uint64_t *n_regions, uint64_t *n_states, void *stream);
int xrs_polygonize_rings(int64_t rows, int64_t cols, const void *work_dev, void *rings_dev, uint64_t n_states,
                         uint64_t n_regions, uint64_t *n_rings, uint64_t *n_points, int *rounds, void *stream);
int xrs_polygonize_scatter(const void *data_dev, int dtype, int64_t rows, int64_t cols, const void *work_dev,
                           const void *rings_dev, uint64_t n_states, uint64_t n_regions, uint64_t n_rings,
                           const double *transform_host, void *points_dev, void *ring_offsets_dev, void *polygon_offsets_dev,
                           void *column_dev, void *stream);

/* rasterize (no counterpart in the reference; the rule is DESIGN.md §6r): polygons burnt into a rows x cols raster (at most
 * 2^32 - 1 cells).  The polygons come as polygonize's flat arrays: points_dev float64 [n_points][2], ring_offsets_dev int64
 * [n_rings + 1], polygon_offsets_dev int64 [n_polygons + 1], non-decreasing, starting at 0 and ending at n_points and n_rings (the
 * caller checks that; rings and polygons may be empty).  Pixel (row j, column i) is the square [i, i + 1] x [j, j + 1]; a cell is
 * inside a polygon when the polygon's crossings of the cell's centre line at or left of the centre are odd in number (even-odd).
 * (polygon, row, column) of a crossing is one 64-bit key: bits(n_polygons - 1) + bits(rows - 1) + bits(cols) <= 64, or the calls
 * fail.  Four calls on one stream, same polygons and shape; the first two wait for the stream once each:
 *   xrs_rasterize_census  inverse_host: NULL (the points are in pixel space) or 6 doubles a0, a1, a2, a3, t2, t5: u = a0 * dx + a1 *
 *              dy, v = a2 * dx + a3 * dy with dx = x - t2, dy = y - t5, products and sums rounded separately.  work_dev:
 *              xrs_rasterize_workspace_size(n_points) bytes, caller-owned.  *n_crossings (host): how often an edge crosses a
 *              row's centre line, always even.  *flags (host): XRS_RASTERIZE_NONFINITE if a vertex is not finite, before or after
 *              the mapping; the other calls must not follow then.  No further call but burn and gather is needed when
 *              *n_crossings is 0.
 *   xrs_rasterize_spans   spans_dev: xrs_rasterize_spans_workspace_size(n_crossings) bytes, caller-owned (0 when n_crossings is 0
 *              or above XRS_RASTERIZE_MAX_CROSSINGS).  *n_spans (host): the spans [c0, c1) of one polygon in one row that are
 *              not empty; *n_items (host): their chunks of 64 columns (aligned to multiples of 64), the work items of burn.
 *   xrs_rasterize_burn    plane_dev: uint32 [rows][cols], cleared by the call; afterwards 0 where no polygon covers the cell, else
 *              1 + the highest priority_dev[p] (uint32 [n_polygons], all different) among the covering polygons, or with `count`
 *              their number.  With n_items == 0 the call only clears the plane, and spans_dev may be NULL.  Does not wait.
 *   xrs_rasterize_gather  out_dev[c] (dtype: XRS_DT_*) = values_dev[order_dev[w - 1]] for w = plane_dev[c] > 0, else *fill_host
 *              (one item of `dtype`); values_dev: [n_polygons] of `dtype`, order_dev: uint32, the polygon of every priority.
 *              With `count`: the plane converted to `dtype`; values_dev, order_dev and the fill are not read.  Does not wait. */
#define XRS_RASTERIZE_MAX_POINTS 2147483647ull
#define XRS_RASTERIZE_MAX_CROSSINGS 2147483646ull
enum { XRS_RASTERIZE_NONFINITE = 1 };
int xrs_rasterize_workspace_size(uint64_t n_points, uint64_t *bytes_out);
int xrs_rasterize_spans_workspace_size(uint64_t n_crossings, uint64_t *bytes_out);
int xrs_rasterize_census(const double *points_dev, const int64_t *ring_offsets_dev, const int64_t *polygon_offsets_dev,
                         uint64_t n_points, uint64_t n_rings, uint64_t n_polygons, int64_t rows, int64_t cols,
                         const double *inverse_host, void *work_dev, uint64_t *n_crossings, int *flags, void *stream);
int xrs_rasterize_spans(const double *points_dev, const int64_t *ring_offsets_dev, const int64_t *polygon_offsets_dev,
                        uint64_t n_points, uint64_t n_rings, uint64_t n_polygons, int64_t rows, int64_t cols,
                        const double *inverse_host, const void *work_dev, void *spans_dev, uint64_t n_crossings,
                        uint64_t *n_spans, uint64_t *n_items, void *stream);
int xrs_rasterize_burn(int64_t rows, int64_t cols, const void *spans_dev, uint64_t n_crossings, uint64_t n_polygons,
                       uint64_t n_items, const uint32_t *priority_dev, int count, uint32_t *plane_dev, void *stream);
int xrs_rasterize_gather(const uint32_t *plane_dev, int64_t rows, int64_t cols, const void *values_dev, const uint32_t *order_dev,
                         int dtype, const void *fill_host, int count, void *out_dev, void *stream);

/* contours (no counterpart in the reference; the rule is DESIGN.md §6s): the isolines of a rows x cols C-contiguous raster
 * (`dtype`: XRS_DT_*, converted to float64; at most XRS_CONTOURS_MAX_CELLS cells) at n_levels levels by marching squares.  Node
 * (r, c) is the centre of cell (r, c), at (c + 0.5, r + 0.5); a node is high where z > level; a quad of four nodes with a corner
 * that is not finite draws nothing; a crossing point belongs to its edge (t = (level - z0) / (z1 - z0) from the edge's upper or
 * left node), so the quads on either side of it get the same bits; saddles go by the centre ((zTL + zTR) + (zBR + zBL)) * 0.25.
 * Three calls on one stream, same raster, shape and levels; the first two wait for the stream (once, and once per group of
 * rounds), the third once:
 *   xrs_contours_census   levels_host: n_levels finite, strictly increasing float64 (else the call fails); the raster is read
 *              once for all of them.  work_dev: xrs_contours_workspace_size(rows, cols, n_levels) bytes, caller-owned.
 *              *n_segments (host): the segments of all quads and levels.  No further call is needed, or allowed, when it is 0
 *              (rows < 2, cols < 2 and n_levels == 0 among the reasons), and none is possible above XRS_CONTOURS_MAX_SEGMENTS.
 *   xrs_contours_lines    lines_dev: xrs_contours_lines_workspace_size(n_segments) bytes, caller-owned.  *n_lines, *n_points
 *              (host): the lines of all levels, and their points: a line of n segments has n + 1, a closed one repeats its first.
 *              rounds (host, 2 words or NULL): the pointer-doubling rounds run to find every line's start and to rank its
 *              segments; each is bounded by 32, beyond which the call fails.
 *   xrs_contours_scatter  sort_dev: xrs_contours_scatter_workspace_size(n_lines) bytes, caller-owned.  transform_host: NULL or 6
 *              doubles, x' = t0 * x + t1 * y + t2, y' = t3 * x + t4 * y + t5 with separately rounded products and sums.
 *              points_dev: float64 [n_points][2]; line_offsets_dev: int64 [n_lines + 1], line i owns points line_offsets[i] ..
 *              line_offsets[i + 1]; level_offsets_dev: int64 [n_levels + 1], level k owns lines level_offsets[k] ..
 *              level_offsets[k + 1], ordered by key (an open line's first edge id, a closed line's smallest, where it begins);
 *              closed_dev: uint8 [n_lines].  Edge ids: 2 * (r * cols + c) for (r, c)-(r, c + 1), one more for (r, c)-(r + 1, c). */
#define XRS_CONTOURS_MAX_CELLS 2147483647ull
#define XRS_CONTOURS_MAX_LEVELS 4194304ull
#define XRS_CONTOURS_MAX_SEGMENTS 4294967294ull
int xrs_contours_workspace_size(int64_t rows, int64_t cols, uint64_t n_levels, uint64_t *bytes_out);
int xrs_contours_lines_workspace_size(uint64_t n_segments, uint64_t *bytes_out);
int xrs_contours_scatter_workspace_size(uint64_t n_lines, uint64_t *bytes_out);
int xrs_contours_census(const void *data_dev, int dtype, int64_t rows, int64_t cols, const double *levels_host, uint64_t n_levels,
                        void *work_dev, uint64_t *n_segments, void *stream);
int xrs_contours_lines(const void *data_dev, int dtype, int64_t rows, int64_t cols, uint64_t n_levels, const void *work_dev,
                       void *lines_dev, uint64_t n_segments, uint64_t *n_lines, uint64_t *n_points, int *rounds, void *stream);
int xrs_contours_scatter(const void *data_dev, int dtype, int64_t rows, int64_t cols, uint64_t n_levels, const void *work_dev,
                         void *lines_dev, void *sort_dev, uint64_t n_segments, uint64_t n_lines, const double *transform_host,
                         void *points_dev, void *line_offsets_dev, void *level_offsets_dev, void *closed_dev, void *stream);

/* idw (no counterpart in the reference; the rule is DESIGN.md §6t): inverse-distance interpolation of n_points scattered points
 * (at most XRS_IDW_MAX_POINTS) onto a rows x cols raster (at most 2^32 - 1 cells) from the exact k nearest neighbours of every
 * cell centre (column + 0.5, row + 0.5), nearest first by (d2, index) with d2 = dx * dx + dy * dy rounded step by step.  The
 * points are sorted into square bins of bin_cells x bin_cells cells (a power of two) plus one apron ring of bins for the points
 * outside; (ceil(cols / bin_cells) + 2) * (ceil(rows / bin_cells) + 2) is at most XRS_IDW_MAX_BINS.  Results never depend on
 * bin_cells.  Two calls on one stream, same n_points, shape and bin_cells:
 *   xrs_idw_bin     points_dev: float64 [n_points][2] (x, y); NULL only with n_points == 0.  inverse_host: as for
 *              xrs_rasterize_census.  work_dev: xrs_idw_workspace_size(n_points, rows, cols, bin_cells) bytes, caller-owned.
 *              *flags (host): XRS_IDW_NONFINITE if a coordinate is not finite, before or after the mapping; the search must
 *              not follow then.  Waits for the stream once.
 *   xrs_idw_search  values_dev: float64 [n_points] by point index (not read without out_dev).  k: 1 .. XRS_IDW_MAX_K; power:
 *              1 .. 8; max_d2: the squared radius in cells, inclusive, or a negative number for none; min_points: 1 .. k, a cell
 *              with fewer candidates gets `fill`.  out_dev: float64 (dtype XRS_DT_F64) or float32 (XRS_DT_F32) [rows][cols], or
 *              NULL.  index_dev: int32 [k][rows][cols], the neighbours' indices, -1 where there is none, or NULL.  d2_dev:
 *              float64 [k][rows][cols], their d2, +inf where there is none, or NULL.  At least one of the three.  Does not wait. */
#define XRS_IDW_MAX_POINTS 2147483647ull
#define XRS_IDW_MAX_BINS 67108864ull
#define XRS_IDW_MAX_K 64
enum { XRS_IDW_NONFINITE = 1 };
int xrs_idw_workspace_size(uint64_t n_points, int64_t rows, int64_t cols, int64_t bin_cells, uint64_t *bytes_out);
int xrs_idw_bin(const double *points_dev, uint64_t n_points, int64_t rows, int64_t cols, int64_t bin_cells,
                const double *inverse_host, void *work_dev, int *flags, void *stream);
int xrs_idw_search(const void *work_dev, const double *values_dev, uint64_t n_points, int64_t rows, int64_t cols,
                   int64_t bin_cells, int k, int power, double max_d2, int min_points, double fill, int dtype, void *out_dev,
                   int32_t *index_dev, double *d2_dev, void *stream);

/* resample (no counterpart in the reference; the rule is DESIGN.md §6u): a src_rows x src_cols C-contiguous raster (`dtype`: any
 * XRS_DT_* code; at most 2^32 - 1 cells and 2^31 - 1 per axis) onto a rows x cols grid (at most 2^32 - 1 cells).  All geometry
 * is in DEVICE TABLES the caller computes, one entry per destination row and one per destination column; the calls only load,
 * compare, multiply, add and divide, in a fixed order.  A tap table of an axis is first_dev: int32 [n] and w_dev: float64
 * [n][taps] (1 .. XRS_RESAMPLE_MAX_TAPS): tap k of destination row (column) i is source row (column) first[i] + k with weight
 * w[i][k].  A tap participates when its weight is not 0.  A tap that does not participate, or whose index lies outside the
 * raster, is never read, whatever the tables hold.  A source cell is valid when it is inside the raster, not NaN and not equal to
 * *nodata_host (one item of `dtype`, or NULL for none).  None of the calls waits.
 *   xrs_resample_gather    out_dev[r][c] (`dtype`) = src[near_y_dev[r]][near_x_dev[c]] (int32 tables), or *fill_host (one item of
 *              `dtype`) where either index is negative or outside the raster, or that cell is invalid.
 *   xrs_resample_weighted  r_j = sum wx[i] * v and n_j = sum wx[i] over the participating valid taps of tap row j, ascending;
 *              num = sum wy[j] * r_j and den = sum wy[j] * n_j over the rows with wy[j] != 0, ascending; float64, every product
 *              and sum rounded on its own, from 0.0.  out_dev[r][c] (`out_dtype`: XRS_DT_F64 or XRS_DT_F32, rounded once) is
 *              num / den with `divide`, else num.  near_y_dev / near_x_dev (both or neither): the cell is `fill` exactly where
 *              xrs_resample_gather's would be; without them, where no valid tap participates.  fb_*: fallback tap tables (all
 *              four or none); with them a cell whose window holds a participating invalid tap is computed from the fallback
 *              tables by the same sums instead.  Up to 8 taps on both axes a workgroup shares the row sums of a tile of cells
 *              through LDS; above, one wave walks one cell.  The result does not depend on which.
 *   xrs_resample_select    op XRS_RESAMPLE_MIN / _MAX: the least / greatest of the participating valid cells of the window, the
 *              first of equals in row-major order; XRS_RESAMPLE_MODE: the value with the most members (classes by ==), the
 *              smaller value on a tie, reported as the class's first member in row-major order; taps_y * taps_x is at most
 *              XRS_RESAMPLE_MODE_MAX_WINDOW for it.  *fill_host where no valid cell participates.  out_dev: `dtype`. */
#define XRS_RESAMPLE_MAX_TAPS 256
#define XRS_RESAMPLE_MODE_MAX_WINDOW 1024
enum { XRS_RESAMPLE_MIN = 0, XRS_RESAMPLE_MAX = 1, XRS_RESAMPLE_MODE = 2 };
int xrs_resample_gather(const void *src_dev, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host, int64_t rows,
                        int64_t cols, const int32_t *near_y_dev, const int32_t *near_x_dev, const void *fill_host, void *out_dev,
                        void *stream);
int xrs_resample_weighted(const void *src_dev, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host, int64_t rows,
                          int64_t cols, const int32_t *first_y_dev, const double *wy_dev, int taps_y, const int32_t *first_x_dev,
                          const double *wx_dev, int taps_x, const int32_t *near_y_dev, const int32_t *near_x_dev,
                          const int32_t *fb_first_y_dev, const double *fb_wy_dev, int fb_taps_y, const int32_t *fb_first_x_dev,
                          const double *fb_wx_dev, int fb_taps_x, int divide, int out_dtype, double fill, void *out_dev,
                          void *stream);
int xrs_resample_select(const void *src_dev, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host, int64_t rows,
                        int64_t cols, const int32_t *first_y_dev, const double *wy_dev, int taps_y, const int32_t *first_x_dev,
                        const double *wx_dev, int taps_x, int op, const void *fill_host, void *out_dev, void *stream);

/* local (xrspatial/local.py): one result per cell from the same cell of n_planes equally sized, C-contiguous planes, each read
 * in its own dtype (XRS_DT_* except XRS_DT_U64).  `planes` and `dtypes` are HOST arrays of n_planes (1 .. XRS_LOCAL_MAX_PLANES)
 * device pointers and codes; they travel in the kernel's argument block.  The rule is DESIGN.md §6f.  The working type is
 * int64 when every plane (and `ref_dev`, where the function reads one) is an integer and the function is not mean, median or
 * std, else float64.
 *   xrs_local_cells   op: XRS_LOCAL_*; ref_dev / ref_dtype: the plane of ref_var for the frequencies, rank and popularity (an
 *                     integer plane for the last two), ignored otherwise.  out_dev: n 8-byte results, int64 if out_is_i64
 *                     (integer working type only; not rank and popularity, which can give NaN), else float64.
 *   xrs_local_combine 1-based ids of the cells' tuples in order of first occurrence, NaN where a plane is NaN, as float64 into
 *                     out_dev; n < 2^31.  First call, first_cells_dev == NULL: computes out_dev and *n_classes and leaves the
 *                     classes' first cells in work_dev (xrs_local_combine_workspace_bytes(n, n_planes) bytes, caller-owned;
 *                     the call synchronises the stream).  Second call, same workspace, first_cells_dev with room for
 *                     first_capacity >= *n_classes entries: copies them there, in id order.
 *   xrs_local_gather  out_dev[t * n_planes + j] = plane j at cell cells_dev[t] as 8 bytes: int64 for an integer plane, float64
 *                     for a floating one (the values of combine's key). */
enum { XRS_LOCAL_MAX_PLANES = 64 };
enum { XRS_LOCAL_MAX = 0, XRS_LOCAL_MIN = 1, XRS_LOCAL_SUM = 2, XRS_LOCAL_MEAN = 3, XRS_LOCAL_STD = 4, XRS_LOCAL_MEDIAN = 5,
       XRS_LOCAL_LESSER = 6, XRS_LOCAL_EQUAL = 7, XRS_LOCAL_GREATER = 8, XRS_LOCAL_LOWEST = 9, XRS_LOCAL_HIGHEST = 10,
       XRS_LOCAL_RANK = 11, XRS_LOCAL_POPULARITY = 12 };
int xrs_local_cells(int op, const void *const *planes, const int *dtypes, int n_planes, const void *ref_dev, int ref_dtype,
                    int64_t n, void *out_dev, int out_is_i64, void *stream);
size_t xrs_local_combine_workspace_bytes(int64_t n, int n_planes);
int xrs_local_combine(const void *const *planes, const int *dtypes, int n_planes, int64_t n, void *work_dev, size_t work_bytes,
                      double *out_dev, unsigned *first_cells_dev, int64_t first_capacity, int64_t *n_classes, void *stream);
int xrs_local_gather(const void *const *planes, const int *dtypes, int n_planes, int64_t n, const unsigned *cells_dev,
                     int64_t n_cells, void *out_dev, void *stream);

/* natural_breaks (xrspatial/classify.py:508-564 `_run_numpy_jenks_matrices`): the two (n + 1) x (k + 1) row-major float32 tables
 * of the Jenks dynamic programme over a sorted float32 sample of n values (1 <= n < 2^24, the limits being float32 row numbers)
 * and k >= 1 classes, initial values included: row 0 and column 0 zero, lower_class_limits[1][1:] = 1, var_combinations[2:][1:] =
 * inf where the sweep leaves them.  Bit for bit the reference's loop: float64 running sums of the float32 values and of their
 * float32 squares, one IEEE float64 division per step, the float32 minimum replaced on `>=`.  One launch for
 * the initial tables, then one per column 1 .. k, one thread per row 2 .. n; n == 1 launches the first only.  work_dev:
 * xrs_jenks_workspace_bytes(n, k) bytes, caller-owned (two contiguous working columns; 0 for arguments the call refuses).
 *   xrs_gather_elems  out_dev[i] = in_dev[idx_dev[i]] for n_idx uint32 indices into n elements of elem_size 1, 2, 4 or 8 bytes,
 *                     copied without conversion (the sample of natural_breaks in the raster's own dtype); an index >= n gives
 *                     zero bytes. */
size_t xrs_jenks_workspace_bytes(int64_t n, int k);
int xrs_jenks_matrices_f32(const float *sorted_dev, int64_t n, int k, float *lower_class_limits_dev, float *var_combinations_dev,
                           void *work_dev, size_t work_bytes, void *stream);
int xrs_gather_elems(const void *in_dev, int elem_size, int64_t n, const uint32_t *idx_dev, int64_t n_idx, void *out_dev,
                     void *stream);

/* bump (xrspatial/bump.py:12-28 `_finish_bump`): out_dev (height x width float64, row-major; zeroed by the call) after the
 * reference's serial loop over `count` bumps -- locs_dev: count (x, y) uint16 pairs, heights_dev: count float64 -- bit for bit: bump
 * i adds its height to its centre, then out[centre] * (d2 / spread^2) to every cell of its clipped footprint (upper bounds
 * exclusive, the centre included with weight 0), every cell's sum taken in bump order, product and add rounded separately.
 * spread <= 0 runs the centre adds only.  Events (cell, bump) are sorted by radix sort and folded in passes that never wait
 * (DESIGN.md 6k); bumps are taken in index-order chunks whose events fit `max_events` (a capacity above count * footprint is cut
 * to that).  Refused before any device work: null pointers, count < 0, width or height < 1, more than 2^31 cells, spread > 2^26, a
 * capacity below one bump's footprint, a workspace below xrs_bump_workspace_bytes (0 for arguments the call refuses).  A location
 * outside the raster is found on the device and reported; nothing is written for it.
 * status (host, 8 int64, may be null): chunks, events, passes, touched cells summed over chunks, then the nanoseconds spent
 * expanding (count, scan, emit), sorting (sort, segment heads) and folding. */
size_t xrs_bump_workspace_bytes(int64_t count, int64_t width, int64_t height, int64_t spread, int64_t max_events);
int xrs_bump_f64(const uint16_t *locs_dev, const double *heights_dev, int64_t count, int64_t width, int64_t height, int64_t spread,
                 double *out_dev, void *work_dev, size_t work_bytes, int64_t max_events, int64_t *status, void *stream);

/* D8 hydrology (no reference counterpart; the rule: xrspatial_amd/hydrology.py).
 *   xrs_flow_direction   out_dev (float32) = the ESRI code (E 1, SE 2, S 4, SW 8, W 16, NW 32, N 64, NE 128) of the neighbour
 *              with the largest drop (float64(z) - float64(zk)) / dist, dist = cellsize_x (E, W), cellsize_y (N, S), diag (the
 *              rest), one IEEE subtraction and one IEEE division; neighbours in the order above, a later one only when its
 *              drop is strictly larger; 0 where no neighbour lies lower, NaN at NaN cells.  `dtype`: XRS_DT_F32 or XRS_DT_F64.
 *              The cell sizes and `diag` (the caller's sqrt(cx^2 + cy^2)) are positive and finite.  One launch.
 *   xrs_flow_accumulate  dir_dev: a float32 plane of such codes (NaN: the cell is outside the graph), at most
 *              XRS_FLOW_MAX_CELLS cells.  acc_out_dev (float64, or NULL): the number of cells whose path reaches the cell, itself
 *              included.  basin_out_dev (float64, or NULL): the linear index of the outlet the cell's path ends in.  Both NaN at
 *              NaN cells.  A cell whose code is 0, or names a neighbour outside the raster or a NaN neighbour, is an outlet.
 *              Pointer doubling: at most (rows * cols).bit_length() rounds, the live pointers counted by every round and read
 *              by the host every two rounds (the call waits for the stream then).
 *   work_dev   xrs_flow_workspace_bytes(rows, cols, want) bytes, caller-owned; `want`: XRS_FLOW_ACCUMULATION | XRS_FLOW_BASINS,
 *              covering the products asked for (0 bytes for an empty raster, one beyond the cell limit or an empty `want`).
 *   status_host HOST array of XRS_FLOW_STATUS_WORDS words: [0] rounds that had live pointers; [1] XRS_FLOW_INVALID_CODE (a
 *              non-NaN value that is no code) | XRS_FLOW_CYCLE (a pointer still live after the bound: the raster holds a cycle)
 *              -- with either bit set the call returns 0 and writes no product; [2], [3] nanoseconds of decode and finish;
 *              [4 + k] live pointers anc_k; [40 + k] nanoseconds of round k.  The times only with XRS_FLOW_TIMED in `flags`
 *              (a stream sync after every launch: tools/hydrology_bench.py). */
enum { XRS_FLOW_ACCUMULATION = 1, XRS_FLOW_BASINS = 2 };
enum { XRS_FLOW_INVALID_CODE = 1, XRS_FLOW_CYCLE = 2 };
enum { XRS_FLOW_TIMED = 1, XRS_FLOW_MAX_ROUNDS = 32, XRS_FLOW_STATUS_WORDS = 80 };
#define XRS_FLOW_MAX_CELLS 0xfffffffeull       /* 2^32 - 2: the all-ones word is the null pointer */
int xrs_flow_direction(const void *data_dev, int dtype, int64_t rows, int64_t cols, double cellsize_x, double cellsize_y, double diag,
                       float *out_dev, void *stream);
size_t xrs_flow_workspace_bytes(int64_t rows, int64_t cols, int want);
int xrs_flow_accumulate(const float *dir_dev, int64_t rows, int64_t cols, void *work_dev, double *acc_out_dev, double *basin_out_dev,
                        int64_t *status_host, int flags, void *stream);

/* Depression fill and flat resolution in front of D8 (the rules: xrspatial_amd/hydrology.py).
 *   xrs_fill        out_dev (z_dev's dtype, another plane than z_dev) = for every cell the least level a path of non-NaN cells
 *              to a rim cell can be held to: z at rim cells (a neighbour outside the raster or NaN), NaN at NaN cells, else the
 *              fixed point of W = max(z, min over the eight neighbours of W) reached from +inf.  Comparisons only.
 *   xrs_flow_flats  code_dev: xrs_flow_direction's result for z_dev, updated in place.  A cell with code 0 that is no rim cell
 *              takes the code of its first neighbour (order E, SE, S, SW, W, NW, N, NE) of equal elevation that is one step
 *              nearer, through cells of that elevation, to a cell with a code or a rim cell; without such a cell it keeps 0.
 *   `dtype`: XRS_DT_F32 or XRS_DT_F64, at most XRS_FLOW_MAX_CELLS cells.  Both relax a plane tile by tile (XRS_FILL_TILE cells
 *   square, in LDS), the tiles coloured 2 x 2 and each colour a launch of its own, in rounds; a round launches the tiles with a
 *   neighbour that changed in the round before; the host reads the count of changed cells after every round (the call waits
 *   for the stream then) and stops at the first 0.  More than rows * cols + 1 rounds are an error.
 *   work_dev   caller-owned; xrs_fill_workspace_size / xrs_flow_flats_workspace_size write its bytes to *bytes_out (0 for an
 *              empty raster or one beyond the cell limit) and return 0, or non-zero for a null pointer.
 *   status_host HOST array of XRS_FILL_STATUS_WORDS words: [0] rounds run, the last one without a change included; [1] tiles
 *              launched in all; [2], [3] nanoseconds of the first and (flats) the last launch; for the first
 *              XRS_FILL_STATUS_ROUNDS rounds k: [8 + k] cells that changed, [8 + ROUNDS + k] tiles launched, [8 + 2 ROUNDS + k]
 *              nanoseconds.  The times only with XRS_FILL_TIMED in `flags` (a stream sync around every launch). */
enum { XRS_FILL_TIMED = 1, XRS_FILL_TILE = 64, XRS_FILL_STATUS_ROUNDS = 80, XRS_FILL_STATUS_WORDS = 256 };
int xrs_fill_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_fill(const void *z_dev, int dtype, int64_t rows, int64_t cols, void *out_dev, void *work_dev, int64_t *status_host, int flags,
             void *stream);
int xrs_flow_flats_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_flow_flats(const void *z_dev, int dtype, int64_t rows, int64_t cols, float *code_dev, void *work_dev, int64_t *status_host,
                   int flags, void *stream);

/* Accumulated least cost from a set of sources over a friction surface (no reference counterpart; the rule:
 * xrspatial_amd/cost_distance.py).
 *   xrs_cost_distance  raster_dev (`dtype`: any XRS_DT_* code) says where the sources are: a source is a cell that is a target
 *              by xrs_proximity's rule (values_dev / values_kind / n_values as there: non-zero and finite with n_values == 0)
 *              and passable.  friction_dev (`friction_dtype`: XRS_DT_F32 or XRS_DT_F64): a cell is passable when its friction
 *              is finite and > 0.  A step between two passable neighbours u, v costs
 *              L * ((float64(f(u)) + float64(f(v))) * 0.5), L = cellsize_x (E, W), cellsize_y (N, S) or diag (the caller's
 *              sqrt(cx^2 + cy^2); only with connectivity 8): one IEEE add, two multiplies.  dist_dev (float64) = the least
 *              plane D with D = 0 at sources and D(v) = min over u of fl(D(u) + w(u, v)), NaN where the cell is impassable,
 *              unreached or D > max_cost.  backlink_dev (float32, or NULL): 0 at sources, NaN where dist_dev is NaN, else the
 *              ESRI code (xrs_flow_direction's) of the first neighbour n with D(n) < D(c) and fl(D(n) + w(n, c)) == D(c).
 *              The plane is relaxed by xrs_fill's schedule (tiles of XRS_FILL_TILE cells square in LDS, 2 x 2 colours, rounds;
 *              the call waits for the stream once a round and at its end).  The result planes are other planes than the inputs.
 *   work_dev   caller-owned; xrs_cost_distance_workspace_size writes its bytes to *bytes_out (0 for an empty raster or one
 *              beyond XRS_FLOW_MAX_CELLS cells) and returns 0, or non-zero for a null pointer.
 *   status_host HOST array of XRS_COST_STATUS_WORDS words, laid out as xrs_fill's: [0] rounds run; [1] tiles launched in all;
 *              [2], [3] nanoseconds of the first launch and of the last two; [4] sources; [5] absorbed cells (reached, no source,
 *              and no neighbour fits the back-link rule: a step was lost to rounding); [6] cells reached, the sources included;
 *              per round k the words [8 + k], [8 + ROUNDS + k], [8 + 2 ROUNDS + k] of xrs_fill.  Times only with XRS_COST_TIMED.
 *   xrs_cost_allocation  out_dev (float32) = float32(raster[b]) where basins_dev (float64: xrs_flow_accumulate's basins of the
 *              back-link plane, the linear index of the source a cell's chain ends in) holds b, NaN where it holds NaN.  One launch. */
enum { XRS_COST_TIMED = 1, XRS_COST_STATUS_WORDS = 256 };
int xrs_cost_distance_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_cost_distance(const void *raster_dev, int dtype, const void *values_dev, int values_kind, int n_values, const void *friction_dev,
                      int friction_dtype, int64_t rows, int64_t cols, double cellsize_x, double cellsize_y, double diag, double max_cost,
                      int connectivity, double *dist_dev, float *backlink_dev, void *work_dev, int64_t *status_host, int flags,
                      void *stream);
int xrs_cost_allocation(const double *basins_dev, const void *raster_dev, int dtype, int64_t rows, int64_t cols, float *out_dev,
                        void *stream);

/* Stream order, stream links, watersheds from pour points and downstream flow length on a raster of D8 codes (no reference
 * counterpart; the rule: xrspatial_amd/hydrology.py).  dir_dev is a float32 plane as xrs_flow_accumulate reads
 * it, at most XRS_FLOW_MAX_CELLS cells; every call runs pointer doubling in at most bit_length rounds, the live pointers counted
 * by every round and read by the host every two rounds (the call waits for the stream then), and no result plane may be an input.
 *   xrs_stream_network  accum_dev (`accum_dtype`: XRS_DT_F32 or XRS_DT_F64): a cell is a stream cell when its code is not NaN and
 *              float64(accum) >= threshold (not NaN).  The stream parent of a stream cell is its downstream cell if that is a
 *              stream cell.  `want`: XRS_STREAM_STRAHLER | XRS_STREAM_SHREVE | XRS_STREAM_LINK, each with its float64 plane
 *              (NaN off the streams; a plane that `want` does not name is not read and may be NULL).  Shreve: the sources of the
 *              upstream stream tree.  Strahler: 1 at a source, else the largest child order m, m + 1 where two children have it.
 *              Link: 1 + the number of link heads (cells with 0 or >= 2 children) in front of the cell's own head in row-major
 *              order, the head of a cell with one child being that child's.  The work runs on the compacted list of stream cells.
 *   status_host (xrs_stream_network) HOST array of XRS_STREAM_STATUS_WORDS words: [0] rounds of the source count; [1]
 *              XRS_FLOW_INVALID_CODE | XRS_FLOW_CYCLE (a ring of stream cells) -- with either set the call returns 0 and writes no
 *              product; [2] Strahler levels (the highest order); [3] stream cells; [4] sources; [5] heads; [6] rounds of the head
 *              jumping; [8] .. [12] nanoseconds of mark + scan + compact, the source count, the Strahler levels, the heads and the
 *              finish (only with XRS_STREAM_TIMED); [16 + r] live parent pointers of round r of the source count; [56 + k] cells
 *              with two or more children of order >= k; [96 + k] rounds of level k.
 *   xrs_flow_watershed  pour_dev (`dtype`: any XRS_DT_* code): a pour point is a cell that is a target by xrs_proximity's rule
 *              (values_dev / values_kind / n_values as there) and whose code is not NaN.  out_dev (float32) = float32(pour[p]) of
 *              the first pour point p on the cell's path, the cell itself included; NaN without one and at NaN cells.
 *   xrs_flow_length  out_dev (float64) = fl(fl(fl(nx * cellsize_x) + fl(ny * cellsize_y)) + fl(nd * diag)), nx / ny / nd the E-W,
 *              N-S and diagonal steps from the cell to its outlet; 0 at outlets, NaN at NaN cells.  Cell sizes positive and finite.
 *   status_host (watershed, length) XRS_FLOW_STATUS_WORDS words laid out as xrs_flow_accumulate's; xrs_flow_watershed adds [37],
 *              the pour points.  Times only with XRS_FLOW_TIMED.
 *   work_dev   caller-owned; the call's *_workspace_size writes its bytes to *bytes_out (0 for an empty raster or one beyond
 *              XRS_FLOW_MAX_CELLS cells) and returns 0, or non-zero for a null pointer. */
enum { XRS_STREAM_STRAHLER = 1, XRS_STREAM_SHREVE = 2, XRS_STREAM_LINK = 4 };
enum { XRS_STREAM_TIMED = 1, XRS_STREAM_STATUS_WORDS = 136 };
int xrs_stream_network_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_stream_network(const float *dir_dev, const void *accum_dev, int accum_dtype, int64_t rows, int64_t cols, double threshold, int want,
                       void *work_dev, double *strahler_out_dev, double *shreve_out_dev, double *link_out_dev, int64_t *status_host, int flags,
                       void *stream);
int xrs_flow_watershed_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_flow_watershed(const float *dir_dev, const void *pour_dev, int dtype, const void *values_dev, int values_kind, int n_values,
                       int64_t rows, int64_t cols, void *work_dev, float *out_dev, int64_t *status_host, int flags, void *stream);
int xrs_flow_length_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_flow_length(const float *dir_dev, int64_t rows, int64_t cols, double cellsize_x, double cellsize_y, double diag, void *work_dev,
                    double *out_dev, int64_t *status_host, int flags, void *stream);

/* D-infinity flow direction and the float accumulation of shares (no reference counterpart; the rule: xrspatial_amd/hydrology.py,
 * DESIGN.md 6q).  The neighbours counter-clockwise from east are n = 0 .. 7: E, NE, N, NW, W, SW, S, SE.  table_host: a HOST array
 * of nine float64, the angles of the neighbours and 2 pi: 0, t, pi/2, pi - t, pi, pi + t, 3 pi/2, 2 pi - t, 2 pi with
 * t = atan2(cellsize_y, cellsize_x); it must start at 0 and be finite and strictly increasing, and is passed on by value.
 *   xrs_flow_direction_dinf  out_dev (float64) = the angle of steepest descent over the eight facets, in radians counter-clockwise
 *              from east (north is row - 1), in [0, 2 pi); -1.0 where xrs_flow_direction gives 0; NaN at NaN cells.  The D8 winner
 *              and `best` come first, as xrs_flow_direction finds them; facet o between neighbours o and o + 1 has the cardinal
 *              neighbour c at d1 and the other cell size d2, s1 = (z - z_c) / d1, s2 = (z_c - z_diag) / d2, and is a candidate iff
 *              s1 > 0, s2 > 0 and fl(s2 d1) < fl(s1 d2); it is taken iff fl(fl(s1 s1) + fl(s2 s2)) > the best square so far
 *              (fl(best best) at first).  codes_dev (float32, or NULL): xrs_flow_direction's codes after xrs_flow_flats; a cell
 *              without a winner gets the table angle of its code there.  `dtype`: XRS_DT_F32 or XRS_DT_F64.  One launch.
 *   xrs_flow_accumulate_frac  dir_dev: with XRS_FLOW_D8 a float32 plane of codes as xrs_flow_accumulate reads it (the receiver's
 *              share is 1.0; table_host may be NULL), with XRS_FLOW_DINF a float64 plane of angles: NaN is outside the graph, -1.0
 *              has no receiver, an angle a in [b[o], b[o + 1]) gives neighbour o the share (b[o + 1] - a) / (b[o + 1] - b[o]) and
 *              neighbour o + 1 the share (a - b[o]) / (b[o + 1] - b[o]), a share that is not > 0 being no edge.  weights_dev
 *              (`weights_dtype`: XRS_DT_F32 or XRS_DT_F64; or NULL: 1.0) is a cell's own contribution w.  acc_out_dev (float64):
 *              acc[v] = w[v], then for the donors u at E, SE, S, SW, W, NW, N, NE of v in this order
 *              acc = fl(acc + fl(share(u -> v) * acc[u])), computed once, when all donors are final; NaN at NaN cells.  The plane is
 *              relaxed by xrs_fill's schedule (tiles of XRS_FILL_TILE cells square, 2 x 2 colours, rounds; the call waits for the
 *              stream once a round); "not final" is a bit of a byte plane in the workspace.
 *   work_dev   caller-owned; xrs_flow_accumulate_frac_workspace_size writes its bytes to *bytes_out (0 for an empty raster or one
 *              beyond XRS_FLOW_MAX_CELLS cells) and returns 0, or non-zero for a null pointer.
 *   status_host HOST array of XRS_FRAC_STATUS_WORDS words laid out as xrs_fill's ([0] rounds, [1] tiles launched, per round k
 *              [8 + k] cells that became final, [8 + ROUNDS + k] tiles, [8 + 2 ROUNDS + k] nanoseconds), and [2], [3] nanoseconds
 *              of the first and the last launch; [4] XRS_FLOW_INVALID_CODE (a value that is neither; found before the rounds) |
 *              XRS_FLOW_CYCLE (a round made no cell final and cells are left: they lie on or below a cycle) -- with either set
 *              the call returns 0 and the plane is no product; [5] the cells left; [6] the cells of the graph.  Times only with
 *              XRS_FRAC_TIMED. */
enum { XRS_FLOW_D8 = 0, XRS_FLOW_DINF = 1 };
enum { XRS_FRAC_TIMED = 1, XRS_FRAC_STATUS_WORDS = 256 };
int xrs_flow_direction_dinf(const void *data_dev, int dtype, int64_t rows, int64_t cols, double cellsize_x, double cellsize_y, double diag,
                            const double *table_host, const float *codes_dev, double *out_dev, void *stream);
int xrs_flow_accumulate_frac_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out);
int xrs_flow_accumulate_frac(const void *dir_dev, int method, const double *table_host, const void *weights_dev, int weights_dtype,
                             int64_t rows, int64_t cols, void *work_dev, double *acc_out_dev, int64_t *status_host, int flags, void *stream);

/* multispectral.true_color (xrspatial/multispectral.py:1334-1495).
 *   xrs_nan_minmax_f32: minmax_dev[0..1] = np.nanmin / np.nanmax of a float32 plane (NaN, NaN if it holds no number);
 *   xrs_true_color_u8:  rgba[i] = { stretch(red), stretch(green), stretch(blue), alpha } with
 *       stretch(v) = uint8( float32( 255 / (1 + exp(c * (th - (v - min) / (max - min)))) ) )   (0 where max == min or NaN)
 *       alpha      = 0 where the red band, in its OWN dtype (`red_raw_dev`, XRS_DT_*), is NaN or <= nodata, else 255;
 *     minmax6_dev = { rmin, rmax, gmin, gmax, bmin, bmax } as produced by xrs_nan_minmax_f32. */
int xrs_nan_minmax_f32(const float *in_dev, int64_t n, float *minmax_dev, void *stream);
int xrs_true_color_u8(const float *red_dev, const float *green_dev, const float *blue_dev, const void *red_raw_dev,
                      int red_raw_dtype, int64_t n, const float *minmax6_dev, double nodata, double c, double th,
                      unsigned char *rgba_dev, void *stream);

/* ----------------------------------------------------- multi-GPU (RCCL, xGMI)
 * One process per GPU.  Rank 0 creates a 128-byte id and ships it to the other
 * ranks by any out-of-band means; every rank then calls xrs_comm_init_rank.
 * halo exchange: the raster is sharded on the row axis; `shard_dev` points at
 * the first OWNED row of this rank's shard, which must have `halo` spare rows
 * above and below it.  One grouped ncclSend/ncclRecv pair per neighbour fills
 * them (rank r-1 above, r+1 below); outer ranks' outer halos are left untouched.
 * zonal reduce: element-wise all-reduce of the partial arrays (sum for
 * count/sum/sumsq, min, max) so every rank holds the global partials; minmax_f64 says
 * whether min_dev / max_dev hold float64 (the *_f64 partials) or float32. */
int xrs_comm_unique_id(void *id128);
int xrs_comm_init_rank(void **comm, const void *id128, int nranks, int rank);
int xrs_comm_destroy(void *comm);
/* {RCCL version code, ranks in the communicator, this rank, HIP device} as RCCL reports them (diagnostics:
 * `bench.py --dry-rccl`; the reference has no counterpart -- dask's scheduler dashboard plays that role) */
int xrs_comm_info(void *comm, int *info4);
int xrs_halo_exchange_f32(void *comm, float *shard_dev, int64_t rows, int64_t cols, int64_t ld,
                          int halo, void *stream);
/* single-GPU loop-back check of the RCCL send/recv plumbing (test support, not on the data path) */
int xrs_comm_selftest_f32(void *comm, const float *src_dev, float *dst_dev, int64_t count, void *stream);
int xrs_zonal_allreduce(void *comm, uint64_t *count_dev, double *sum_dev, double *sumsq_dev,
                        void *min_dev, void *max_dev, int minmax_f64, int n_zones, void *stream);
/* plain typed all-reduce of a device buffer, in place; op: 0 = sum, 1 = min, 2 = max.  Control-plane values of the
 * sharded operators (what dask's scheduler moves for the reference: the zone-id range and the presence map of
 * zonal.stats, zonal.py:181-277; the global moments of hotspots, focal.py:940-984) and the benchmark's barrier. */
int xrs_allreduce_f64(void *comm, double *buf_dev, int64_t count, int op, void *stream);
int xrs_allreduce_u8(void *comm, uint8_t *buf_dev, int64_t count, int op, void *stream);
int xrs_allreduce_u64(void *comm, uint64_t *buf_dev, int64_t count, int op, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XRS_HIP_H */
