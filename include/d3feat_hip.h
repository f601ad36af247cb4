/* d3feat_hip.h -- C ABI of libd3feat_hip.so, the MI355X (gfx950) implementation of the D3Feat hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - all tensors are dense row-major; point clouds are [N,3] float32, features [N,C] float32,
 *     neighbor tables [Nq,H] int32 with the reference's shadow convention: entry == Ns (number of
 *     support rows) means "no neighbor" (reference neighbors.cpp:324, blocks.py:277,356);
 *   - batch (stack) lengths are int32 device arrays of B entries, like the reference's q_batches /
 *     s_batches (cpp_neighbors/wrapper.cpp:85-86);
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous and stream-ordered, never
 *     synchronise, never allocate; scratch comes from the caller (`ws`, size from *_ws_bytes);
 *   - return value: 0 on success, negative D3F_E* on a host-detectable argument error.  Device-detected
 *     conditions (candidate overflow, cell-range overflow) are OR-ed into the int32 status word the
 *     caller supplies; the Python layer maps both to RuntimeError, the reference's only error type
 *     (cpp_neighbors/wrapper.cpp:77,95,...).
 *
 * Each entry point names the reference interface it replaces.
 */
#ifndef D3FEAT_HIP_H_
#define D3FEAT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3F_OK 0
#define D3F_EINVAL (-1)     /* bad argument (shape / null / unsupported size) */
#define D3F_EWORKSPACE (-2) /* workspace too small */
#define D3F_ELAUNCH (-3)    /* HIP launch failure */

/* bits of the device status word */
#define D3F_ST_CAND_OVERFLOW 1  /* a query had more in-radius candidates than the kernel can rank */
#define D3F_ST_CELL_RANGE 2     /* a point fell outside the +-32767-cell addressable grid */
#define D3F_ST_TABLE_FULL 4     /* voxel hash table full (workspace sized for fewer points) */
#define D3F_ST_CAPACITY 8       /* an output needed more rows than the caller's capacity */
#define D3F_ST_WIDE_OVERFLOW 16 /* a point has more in-radius neighbors than the wide (reverse) table holds */
#define D3F_ST_NO_NEAREST 32    /* d3f_radius_query_prefix with a nearest bound: a query has no support within the bound */

const char* d3f_version(void);
int d3f_device_arch_ok(void); /* 1 if the current HIP device is gfx950, 0 otherwise, <0 = -(hipError_t) */
int d3f_device_arch_name(char* out, int n); /* gcnArchName of the current device */
void d3f_debug_set_flags(int flags);      /* profiling aid: ablation switches of the fused KPConv kernels (0 = off) */
/* measurement aid (profiles/phase_clock.py): `counters` = device uint64 buffer (or NULL to switch it off): [0] = waves
 * recorded (cleared by the caller), [1] = record capacity, record r at [8 + 8 r .. +5] = shader cycles one wave of the
 * fused KPConv forward / gather-form grad-input kernel spent in each of its phases (see the kernels). */
void d3f_debug_set_phase_clock(void* counters);
/* measurement aid (bench.py roofline leg): HIP events on the launch stream around every launch of ONE kernel
 * (which = 1 fused KPConv forward kernel, 2 scatter-form grad-input kernel, 3 gather-form grad-input kernel, 4 the
 * A^T B weight-gradient kernels launched one problem at a time, 5 / 6 the forward / transposed KPConv aggregation
 * kernels, 7 the GROUPED A^T B weight-gradient launches (d3f_linear_grad_weight_group: one record per group, both
 * launches); or, negative, minus a bit mask of several: -(1 | 2 | ... | 64)) between begin and end.  end -- after the
 * caller synchronised the device -- returns the number of launches seen and fills ms_out[i] and
 * shapes_out[6*i .. 6*i+5] = {Nq, Ns, H, Cin, Cout, K | which << 8} for the first `cap` of them (which = 7:
 * {problems, sum of 2 R M N in MiFLOP, sum of 4 R (M + N) + 4 M N in KiB, workgroups, 0, 7 << 8}). */
int d3f_debug_kernel_timing_begin(int which, int max_launches);
int d3f_debug_kernel_timing_end(float* ms_out, int32_t* shapes_out, int cap);

/* Tunables of the library -- ONE struct instead of environment variables: the library itself never reads the
 * environment.  d3f_get_tunables fills the current values (defaults at load), d3f_set_tunables replaces them all
 * (process-wide; set them before the launches they concern, not concurrently with them).  The experiment scripts under
 * profiles/ and the tests are the only callers; 0 = "the built-in choice" for every field. */
typedef struct d3f_tunables {
  int32_t atb_task_us;        /* grouped A^T B: modelled duration of one workgroup's task in us (0 = 40) */
  int32_t atb_form;           /* one-problem weight gradients: 0 = by size, 1 = always the first (direct-load) form,
                               * 2 = always the grouped (LDS-DMA ring) kernels */
  int32_t atb_first_form_wgs; /* first form: workgroups along the reduction (0 = by shape) */
  int32_t match_wgs;          /* d3f_mutual_nn: target number of workgroups (0 = 2048) */
  int32_t agg_through_lds;    /* general-path KPConv aggregation: 1 = stage the tile through LDS (experiment) */
  int32_t atb_pipe;           /* grouped A^T B task body: 0 = software-pipelined, 1 = the plain one, n >= 2 = pipelined only for
                               * tiles of at least n 16x16 accumulators (A/B measurements) */
  int32_t xw_rows;            /* d3f_gemm_epilogue: 0 = by shape, 2 / 4 = 32- / 64-row output blocks (A/B measurements) */
  int32_t xw_split;           /* d3f_gemm_epilogue: 0 = by shape, 1 = never split the reduction, 8 q = 8 q partitions */
  int32_t rowgemm_wide;       /* row-streaming unary kernels, 4 consecutive columns per lane at 64 / 128 outputs: 0 = from 65536 rows,
                               * 1 = never, 2 = always (A/B measurements) */
  int32_t rowgemm_rt;         /* forward row-streaming unary kernels with the weights in registers over two row tiles per wave:
                               * 0 = from 4096 rows at reductions of 16 / 32 / 64, 1 = never (A/B measurements) */
  int32_t reserved[6];
} d3f_tunables;
void d3f_get_tunables(d3f_tunables* out);
int d3f_set_tunables(const d3f_tunables* in);

/* ------------------------------------------------------------------------------------------------
 * Radius neighbors -- replaces radius_neighbors.batch_query
 *   (cpp_wrappers/cpp_neighbors/wrapper.cpp:58-238 -> neighbors/neighbors.cpp:211-333) and the column
 *   truncation of datasets/dataloader.py:52-67 (batch_neighbors_kpconv).
 * One uniform cell list ("grid") is built per support cloud + radius and can serve several query sets
 * (conv, pool and upsample searches of one pyramid level share it).
 * ---------------------------------------------------------------------------------------------- */
size_t d3f_radius_grid_ws_bytes(int Ns);
/* Build the cell list of `supports` for `radius` into grid_ws. */
int d3f_radius_grid_build(const float* supports, int Ns, const int32_t* s_len, int B, float radius,
                          void* grid_ws, size_t grid_ws_bytes, int32_t* status, void* stream);
/* A pyramid build clears the bucket counters of its five cell lists (the first d3f_radius_grid_zero_bytes(Ns) bytes of each
 * grid_ws) and its per-table counters with ONE launch (d3f_zero_buffers, up to 8 buffers of 4-byte multiples) and builds
 * the lists with d3f_radius_grid_build_prezeroed. */
size_t d3f_radius_grid_zero_bytes(int Ns);
int d3f_zero_buffers(void* const* ptrs, const size_t* bytes, int n, void* stream);
/* One launch for the inputs of a (stacked) training step -- the dataset item of reference datasets/ThreeDMatch.py:135-149:
 * kinds[j] = 0 copies bytes[j] (4-byte multiple) srcs[j] -> dsts[j] on the device; 1 writes the circle loss's mask
 * dsts[j][i] (uint8) = srcs[j][i] (float64 dist_keypts) > threshold (utils/loss.py:119), i < bytes[j] / 8.  n <= 24. */
int d3f_copy_buffers(const void* const* srcs, void* const* dsts, const size_t* bytes, const int* kinds, int n,
                     double threshold, void* stream);
/* d3f_radius_query_prefix for the rows nobody has filled yet: a row q with done_rows[q] > 0 is left untouched. */
int d3f_radius_query_prefix_missing(const void* grid_ws, const float* queries, int Nq, const int32_t* q_len, int Ns,
                                    const int32_t* s_len, int B, float grid_radius, float radius, float prefix_radius,
                                    float nearest_bound, int width, int32_t* out_idx, const int32_t* done_rows,
                                    int32_t* status, void* stream);
/* A pooling search (coarse queries over the fine cloud, reference datasets/dataloader.py:141-146) that leaves its TRANSPOSE
 * behind: capped table, max count(s) and last kept keys as d3f_radius_query_ex, and every fine point f found within the
 * radius of coarse query c gets the key (d2 bits << 32 | c) appended to tr_keys[32 f ...] (scratch of 32 Ns uint64),
 * tr_counts[f] [Ns] int32 (cleared by the caller) counting them.  These are the pairs of the upsampling search at the same
 * radius seen from the fine side, with the same distance bits.  A list that outgrows its 32 slots keeps counting (the
 * ranking drops it and the row is searched for). */
int d3f_radius_query_pool_transposed(const void* grid_ws, const float* queries, int Nq, const int32_t* q_len, int Ns,
                                     const int32_t* s_len, int B, float grid_radius, float radius, int width,
                                     int32_t* out_idx, int32_t* max_count, uint64_t* out_last_key, int max_count_group,
                                     int32_t* tr_counts, uint64_t* tr_keys, int32_t* status, void* stream);
/* The training engine's upsampling rows (prefix form: the coarse points within the POOLING radius of every fine point,
 * ranked by (d2, index): dataloader.py:147-152 restricted to what closest_pool, models/blocks.py:79-91, and the transposed
 * pooling table read) ranked from those lists: rows of `up` [Nf, width] (shadow = Nc) with at least one key are written;
 * rows with counts[f] == 0 (the fine point's own voxel barycentre lies farther than the pooling radius; padding rows) are
 * for d3f_radius_query_prefix_missing, and so are the rows whose list outgrew its 32 slots: counts[f] is set back to 0. */
int d3f_upsample_rows_rank(int32_t* counts, const uint64_t* keys, int Nf, int Nc, int width, int32_t* up,
                           void* stream);
int d3f_radius_grid_build_prezeroed(const float* supports, int Ns, const int32_t* s_len, int B, float radius,
                                    void* grid_ws, size_t grid_ws_bytes, int32_t* status, void* stream);
/* Query: out_idx [Nq,width] gets, per query, the in-radius supports of the same batch element, ordered by
 * (d2, index) ascending, first `width` kept, padded with Ns.  out_counts [Nq] (optional) = uncapped count;
 * max_count (optional, 1 int32, caller-zeroed) = max over queries.  d2 arithmetic and the strict d2 < r2 test
 * follow nanoflann.hpp:433-441,249-251 bit for bit. */
int d3f_radius_query(const void* grid_ws, const float* queries, int Nq, const int32_t* q_len,
                     const float* supports, int Ns, const int32_t* s_len, int B, float radius, int width,
                     int32_t* out_idx, int32_t* out_counts, int32_t* max_count, int32_t* status, void* stream);

/* Extended query.  radius <= grid_radius: a search with a smaller radius on a cell list built for grid_radius (the
 * 27-cell scan is a superset).  Optional extra outputs, for the gather-form KPConv grad-input (no reference
 * counterpart -- autograd scatters):
 *   out_wide [Nq, wide_width]: the WHOLE ranked list of every query, padded with Ns (more than wide_width entries
 *     sets D3F_ST_WIDE_OVERFLOW);
 *   out_last_key [Nq] uint64: rank key (d2 bits << 32 | index) of the last entry the capped row (width) keeps, ~0 when
 *     the row keeps every candidate.  s is listed by query q  <=>  d2(q,s) < r2 and key(q,s) <= last_key[q], which
 *     makes the wide list of a point s over the QUERY cloud, filtered by that test, the transpose of the capped
 *     table (the in-radius relation is symmetric and d2 is bit-identical both ways).
 *   max_count_group > 0: max_count is an array of ceil(B / max_count_group) words, one per group of that many
 *     consecutive clouds (8 stacked pairs -> the max count each pair's own table would have had); 0: one word. */
int d3f_radius_query_ex(const void* grid_ws, const float* queries, int Nq, const int32_t* q_len, int Ns,
                        const int32_t* s_len, int B, float grid_radius, float radius, int width, int32_t* out_idx,
                        int32_t* out_counts, int32_t* max_count, int32_t* out_wide, int wide_width,
                        uint64_t* out_last_key, int max_count_group, int32_t* status, void* stream);
/* Prefix form of a search, for the upsampling tables INSIDE the training engine (datasets/dataloader.py:148-150 builds
 * them with radius 2 r; the network reads column 0, models/blocks.py:79-91, and this build reads the transpose of the
 * pooling table off their leading part): row q = the supports within prefix_radius of q, ranked exactly like the leading
 * part of the d3f_radius_query row, or -- when there is none -- the single nearest support within `radius`.  The entries
 * between the two radii are neither ranked nor stored.  collate_fn_descriptor's tables keep the full rows.
 * nearest_bound (0: none; else prefix_radius <= nearest_bound <= radius): the caller's guarantee that every query has a
 * support within that distance -- a fine point lies within the voxel diagonal 0.8 r sqrt(3) < 1.5 r of its own voxel's
 * barycentre, the coarse point it was subsampled into (dataloader.py:141-146) -- so cells beyond it are not scanned. */
int d3f_radius_query_prefix(const void* grid_ws, const float* queries, int Nq, const int32_t* q_len, int Ns,
                            const int32_t* s_len, int B, float grid_radius, float radius, float prefix_radius,
                            float nearest_bound, int width, int32_t* out_idx, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Grid subsampling -- replaces grid_subsampling.subsample_batch, points-only branch
 *   (cpp_wrappers/cpp_subsampling/wrapper.cpp:62-333 -> grid_subsampling/grid_subsampling.cpp:5-211),
 *   i.e. batch_grid_subsampling_kpconv (datasets/dataloader.py:12-22).
 * order: D3F_ORDER_REFERENCE reproduces the reference's row order (iteration order of the libstdc++
 *   std::unordered_map<size_t,...> it accumulates into, grid_subsampling.cpp:48,85);
 *   D3F_ORDER_FIRST_SEEN emits cells in order of their first input point (cheaper).
 * N is a row CAPACITY: only the first sum(len) rows are read, so levels can be chained without reading
 * lengths back to the host.  Outputs: out_points [out_cap,3] (rows past the emitted total are zero-filled; a total
 * above out_cap sets D3F_ST_CAPACITY), out_len [B], out_total [1].
 * ---------------------------------------------------------------------------------------------- */
#define D3F_ORDER_REFERENCE 0
#define D3F_ORDER_FIRST_SEEN 1
size_t d3f_grid_subsample_ws_bytes(int N, int B);
int d3f_grid_subsample(const float* points, int N, const int32_t* len, int B, float sampleDl, int max_p, int order,
                       float* out_points, int out_cap /* rows of out_points; <= 0: N */, int32_t* out_len,
                       int32_t* out_total, void* ws, size_t ws_bytes, int32_t* status, void* stream);
/* The same call with the reference's optional per-point features [N,fdim] (float) and classes [N,ldim] (int) --
 *   subsample_batch(points, batches, features=, classes=) (wrapper.cpp:75-82,240-247; datasets/dataloader.py:24-50).
 *   out_features [out_cap,fdim] = sequential float32 sum of the cell's member features in input order / (float)count
 *   (grid_subsampling.h:50, .cpp:89-95); out_classes [out_cap,ldim] = per column the value with the most votes, ties
 *   resolved like the reference's std::max_element over its std::unordered_map<int,int> (.cpp:97-102).  Either input
 *   may be NULL (that output is then not written).  Rows follow out_points (same order, same max_p truncation).
 *   NOTE reference bug kept out: with ldim > 1 AND more than one cloud the reference slices the classes of clouds
 *   b > 0 with a wrong end iterator (.cpp:157-158, undefined behaviour); this entry point slices correctly. */
int d3f_grid_subsample_ex(const float* points, int N, const int32_t* len, int B, float sampleDl, int max_p, int order,
                          const float* features, int fdim, const int32_t* classes, int ldim, float* out_points,
                          int out_cap, int32_t* out_len, int32_t* out_total, float* out_features, int32_t* out_classes,
                          void* ws, size_t ws_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * KPConv -- replaces models/blocks.py:237-382 (KPConv.forward, rigid / 'linear' / 'sum' path) and its
 *   autograd backward.
 *   out[n,:] = ( sum_k ( sum_h w[n,h,k] * x[idx[n,h],:] ) @ W[k] ) / nn[n]
 *   w = max(0, 1 - |(s[idx[n,h]] - q[n]) - kp[k]| / extent),  nn[n] = max(1, #{h : sum_c x[idx[n,h],c] > 0})
 * nn_out [Nq] float32 is saved for the backward pass.
 * wf_save (optional, [Nq, d3f_kpconv_saves_wf(...)] float32): the weighted features sum_h w[n,h,k] x[idx[n,h],c] are
 *   left there for the backward pass (what autograd keeps alive in the reference as `weighted_features`,
 *   blocks.py:375).  d3f_kpconv_saves_wf returns the floats per query: K*Cin, except for the Cin <= 4 input-layer
 *   kernels, whose rows are padded to 16 kernel-point slots (16*Cin; slots >= K are zero), and 0 when nothing is saved.
 * spack_keep (optional, 16*Ns bytes) / grad_x_clear (optional, [Ns, Cin]): the forward packs the supports as
 *   float4 {x, y, z, [sum_c feat > 0]}; with spack_keep the packed array is left in the caller's buffer and handed
 *   back to the backward pass (spack_kept), which then launches no packing kernel of its own; grad_x_clear is the
 *   backward's scatter target, cleared here on the side (pass grad_x_precleared = 1 to the backward).  Honoured when
 *   d3f_kpconv_packs_supports says so (otherwise pass NULL / 0).
 *   grad_x_clear == D3F_SPACK_READY: spack_keep ALREADY holds the packed supports of (s_pts, x) -- written by the
 *   epilogue that produced x (d3f_bias_act_forward, spack_out) -- and whatever needed clearing was cleared there; the
 *   forward then launches no packing kernel at all.  Same convention for d3f_kpconv_aggregate.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_SPACK_READY ((float*)(uintptr_t)1)
int d3f_kpconv_forward(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                       const float* x, int Cin, const float* kernel_points, int K, const float* weights, int Cout,
                       float extent, float* out, float* nn_out, float* wf_save, void* spack_keep, float* grad_x_clear,
                       void* ws, size_t ws_bytes, void* stream);
int d3f_kpconv_saves_wf(int Cin, int Cout, int K, int H);
int d3f_kpconv_packs_supports(int Cin, int Cout, int K, int H, int Ns);
size_t d3f_kpconv_ws_bytes(int Nq, int Ns, int H, int K, int Cin, int Cout);
/* grad_x [Ns,Cin] and grad_w [K,Cin,Cout] are OVERWRITTEN.  wf_saved (optional): the forward's wf_save; without it
 * the aggregation is recomputed. */
int d3f_kpconv_backward(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                        const float* x, int Cin, const float* kernel_points, int K, const float* weights, int Cout,
                        float extent, const float* nn, const float* grad_out, const float* wf_saved,
                        const void* spack_kept, int grad_x_precleared, float* grad_x, float* grad_w, void* ws,
                        size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Reverse neighbor table + gather-form grad-input of KPConv -- replaces the scatter-add (index_add_) autograd runs
 *   for the gathers of models/blocks.py:277-280,356-359 in backward.
 * d3f_reverse_table_build: CSR transpose of idx [Nq,H] over Ns supports (entries outside [0,Ns) are shadow):
 *   rev_ent[rev_ptr[s] .. rev_ptr[s+1]) = the queries that list support s, ascending; rev_ptr [Ns+1], rev_ent [Nq*H].
 *   Deterministic.  Built once per table (next to the radius search) and reused by every layer on that table.
 * d3f_kpconv_grad_input_gather: grad_x [Ns,Cin] = sum_k (sum_{q in rev(s)} w(q,s,k) grad_out[q,:]/nn[q]) @ W[k]^T
 *   (OVERWRITTEN; no atomics, bit-reproducible).  nn may be NULL (grad_out already divided).  rev(s) comes in one of
 *   three forms: the exact form rev_rel (below), CSR (rev_ptr + rev_ent, rev_last_key NULL) or the search's own output
 *   (rev_ptr NULL): rev_ent =
 *   out_wide [Ns, rev_width] of a d3f_radius_query_ex of the SUPPORT points over the QUERY cloud with the table's
 *   radius, rev_last_key = out_last_key [Nq] of the query that produced the table -- no transposition pass at all.
 *   rev_radius > 0: rev_ent comes from a search with a LARGER radius (a pooling table's transpose is the prefix, within
 *   the pooling radius rev_radius, of the rows of the upsampling table the pyramid holds anyway: radius 2r, ranked by
 *   distance); a full row whose last entry is still within rev_radius sets D3F_ST_WIDE_OVERFLOW in status (optional).
 * ---------------------------------------------------------------------------------------------- */
size_t d3f_reverse_table_ws_bytes(int Nq, int H, int Ns);
int d3f_reverse_table_build(const int32_t* idx, int Nq, int H, int Ns, int32_t* rev_ptr, int32_t* rev_ent, void* ws,
                            size_t ws_bytes, void* stream);
int d3f_kpconv_grad_input_gather_supported(int Cin, int Cout, int K);
int d3f_kpconv_grad_input_gather(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* rev_ptr,
                                 const int32_t* rev_ent, const uint64_t* rev_last_key, int rev_width, float rev_radius,
                                 const float* rev_rel, const float* kernel_points, int K, const float* weights, int Cin,
                                 int Cout, float extent, const float* nn, const float* grad_out, float* grad_x,
                                 int32_t* status, void* stream);
/* d3f_reverse_table_filter: search form -> EXACT form, once per table in the pyramid build: rev_rel_out [Ns, rev_width]
 * float4 {q - s, bits of q} = the entries of row s that pass the membership test (key <= rev_last_key[q], and d2 <
 * rev_radius^2 when rev_radius > 0), compacted in rank order, rows padded with index Nq.  d3f_kpconv_grad_input_gather
 * with rev_rel (rev_ptr / rev_ent / rev_last_key NULL) then reads each neighborhood as one coalesced run: no position
 * or key gathers, no membership test on the training stream. */
int d3f_reverse_table_filter(const int32_t* rev_ent, int rev_width, const uint64_t* rev_last_key, const float* q_pts,
                             int Nq, const float* s_pts, int Ns, float rev_radius, float* rev_rel_out, int32_t* status,
                             void* stream);

/* grad_x alone, from gwf = (grad_out / nn) @ W^T  [Nq, K*Cin] computed by the caller (an ordinary GEMM: the right
 * tool for the few-point / 256..512-channel layers at the bottom of the U-Net, where the fused kernel's own gW tile
 * would run on a handful of workgroups).  Same semantics as the grad_x of d3f_kpconv_backward.
 * Workspace: d3f_kpconv_ws_bytes(Nq, Ns, H, K, Cin, 64). */
int d3f_kpconv_grad_input_supported(int Cin, int K, int H, int Ns);
/* forward counterpart for the same layers: only the neighbor aggregation wf [Nq, K*Cin] and nn [Nq]; the caller
 * computes out = (wf @ W) / nn with a GEMM (and d3f_bias_act_forward's row_div). */
int d3f_kpconv_aggregate(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                         const float* x, int Cin, const float* kernel_points, int K, float extent, float* wf_out,
                         float* nn_out, void* spack_keep, float* grad_x_clear, void* ws, size_t ws_bytes,
                         void* stream);
int d3f_kpconv_grad_input(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                          const float* x, int Cin, const float* kernel_points, int K, float extent, const float* gwf,
                          const void* spack_kept, int grad_x_precleared, float* grad_x, void* ws, size_t ws_bytes,
                          void* stream);
/* The aggregation of d3f_kpconv_aggregate on the TRANSPOSED graph (autograd of models/blocks.py:359-380 with the sums
 * over queries and over (kernel point, output channel) exchanged):
 *   agg_out [Ns, K*Cout],  agg_out[s, k, o] = sum_{q lists s} w(q, s, k) * grad_out[q, o] (/ nn[q] when nn != NULL)
 * over the exact-form reverse table of d3f_reverse_table_filter (rev_rel [Ns, rev_width, 4]); the caller's GEMM
 *   grad_x [Ns, Cin] = agg_out @ W',  W'[k*Cout + o, c] = weights[k, c, o]
 * finishes the grad-input without atomics (every row written once, bit-reproducible).  Registers -> HBM, no LDS tile:
 * the wide layers (>= 64 channels), whose contraction dominates, run it as a tall library GEMM instead of inside the
 * fused gather kernel.  Every row of agg_out is written (rows without reverse neighbors get zeros). */
int d3f_kpconv_aggregate_transposed_supported(int Cout, int K);
int d3f_kpconv_aggregate_transposed(const float* rev_rel, int rev_width, int Ns, int Nq, const float* kernel_points,
                                    int K, float extent, const float* nn, const float* grad_out, int Cout,
                                    float* agg_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weight gradient of the 1x1 "unary" convolutions -- replaces autograd's grad_out^T @ x for nn.Linear in
 * UnaryBlock (models/blocks.py:481-515): grad_w [Cout, Cin] = grad_out^T [Cout, N] @ x [N, Cin], with the
 * reduction over the N points spread over the chip (deterministic two-pass sum, no atomics).
 * Supported when Cin and Cout are multiples of 16 (d3f_linear_grad_weight_supported).
 * ---------------------------------------------------------------------------------------------- */
int d3f_linear_grad_weight_supported(int N, int Cin, int Cout);
/* The same blocks at the upper pyramid levels (many rows, Cin/Cout <= 256): x W^T with the epilogue
 * act(. + bias1 + add + bias2) applied before the only store, and grad_x = grad_out W, as row-streaming f32-MFMA
 * kernels (a library GEMM is launch-bound on these shapes).  Supported: Cin, Cout in {32, 64, 128, 256} on the output
 * side, a multiple of 16 up to 1024 on the reduction side (d3f_linear_fused_supported checks both directions). */
int d3f_linear_fused_supported(int N, int Cin, int Cout);
int d3f_linear_bias_act_forward(const float* x, const float* weight, int N, int Cin, int Cout, const float* bias1,
                                const float* add, const float* bias2, float slope, float* out, float* zero_init,
                                int zero_n, void* stream);
/* The last unary block of a bottleneck AND its shortcut unary in one launch (models/blocks.py:658-686: unary2(x),
 * unary_shortcut(features), leaky_relu(x + shortcut)): out = act(x1 w1^T + x2 w2^T + bias1 + bias2 + bias3 + bias4); the
 * [N, Cout] shortcut tensor is never formed.  Served while both weight matrices stay in registers
 * (d3f_linear_pair_supported: from 4096 rows, (Cin1 | Cin2) -> Cout = (32 | 64) -> 128 or (16 | 32) -> 64). */
int d3f_linear_pair_supported(int N, int Cin1, int Cin2, int Cout);
int d3f_linear_pair_bias_act_forward(const float* x1, const float* w1, int Cin1, const float* x2, const float* w2, int Cin2,
                                     int N, int Cout, const float* bias1, const float* bias2, const float* bias3,
                                     const float* bias4, float slope, float* out, float* zero_init, int zero_n,
                                     void* stream);
/* grad_x [N,Cin] = grad_out [N,Cout] @ weight [Cout,Cin] (+ add [N,Cin] when given: the gradient another branch
 * produced for the same tensor, accumulated in the epilogue instead of by a separate launch) */
int d3f_linear_grad_input(const float* grad_out, const float* weight, int N, int Cin, int Cout, const float* add,
                          float* grad_x, void* stream);
/* W'[k][o][c] = W[k][c][o] for up to 16 KPConv weight tensors [K, Cin, Cout] in ONE launch (Cin, Cout multiples of 32):
 * the permuted matrices the transposed-aggregation grad-input contracts with -- autograd's grad of
 * torch.matmul(weighted_features, self.weights) (models/blocks.py:369-374) w.r.t. the features, seen from the supports.
 * All pointer / size arrays are HOST arrays of n entries; the tensors are device memory. */
int d3f_permute_kpconv_weights(const float* const* srcs_host, float* const* dsts_host, const int* K_host,
                               const int* Cin_host, const int* Cout_host, int n, void* stream);
/* The contractions of the wide / few-row layers with their epilogue, y [R,N] = act(x [R,K] . B / row_div + bias1 + add +
 * bias2), as ONE f32-MFMA launch (two when the reduction is split: few rows against a long reduction) -- what the
 * reference computes as torch.matmul followed by separate bias / residual / LeakyReLU ops:
 *   KPConv's `torch.matmul(weighted_features, self.weights)` summed over kernel points (models/blocks.py:362-374) with
 *   the /neighbor-count of :376-380 and the bias + LeakyReLU of :473,:598,:676 (mode 1, B = weights viewed [K Cin, Cout],
 *   row_div = neighbor counts); nn.Linear of UnaryBlock (:481-541, y = x W^T: mode 0, B = weight [N, K]) with the
 *   residual add of :686; and autograd's grad-input products g W (mode 1) / g W^T (mode 0).
 * mode 0: B [N, ldw] reduction-contiguous (rows = output columns); kblock > 0: B is [K / kblock][N][kblock] -- the
 *   reduction index b kblock + o of output column n lives at w + (b N + n) kblock + o, i.e. KPConv's weights
 *   [K, Cin, Cout] read as the permuted matrix W'[k, o, c] = W[k, c, o] of the transposed-aggregation grad-input
 *   (ldw is ignored).
 * mode 1: B [K, ldw] (rows = reduction indices).
 * K and N multiples of 16; x, w, y, add, biases 16-byte aligned, leading dimensions multiples of 4.  row_div / bias1 /
 * add [R, ldadd] / bias2 optional, slope = 1: no activation.  zero_init / zero_n as in d3f_bias_act_forward.
 * ws >= d3f_gemm_epilogue_ws_bytes(R, K, N) (slabs of a split reduction; may be 256 bytes).  Bit-reproducible. */
int d3f_gemm_epilogue_supported(int R, int K, int N, int mode, int kblock);
size_t d3f_gemm_epilogue_ws_bytes(int R, int K, int N);
int d3f_gemm_epilogue(const float* x, int ldx, const float* w, int ldw, int mode, int kblock, int R, int K, int N,
                      const float* row_div, const float* bias1, const float* add, int ldadd, const float* bias2,
                      float slope, float* y, int ldy, float* zero_init, int zero_n, void* ws, size_t ws_bytes,
                      void* stream);
size_t d3f_linear_grad_weight_ws_bytes(int N, int Cin, int Cout);
int d3f_linear_grad_weight(const float* x, const float* grad_out, int N, int Cin, int Cout, float* grad_w, void* ws,
                           size_t ws_bytes, void* stream);
/* The same, and the second-stage launch (the fixed-order sum of the partial gradient slabs) also finishes the bias
 * gradient of the block -- autograd's grad_out.sum(0) for the bias of nn.Linear / BatchNormBlock's bias
 * (models/blocks.py:473,497): grad_bias[c] (and grad_bias2[c], optional) = sum_b bias_part[b][c] over the
 * bias_blocks x bias_cols partial column sums d3f_bias_act_backward_partial wrote. */
int d3f_linear_grad_weight_bias(const float* x, const float* grad_out, int N, int Cin, int Cout, float* grad_w, void* ws,
                                size_t ws_bytes, const float* bias_part, int bias_blocks, int bias_cols,
                                float* grad_bias, float* grad_bias2, void* stream);
/* ALL weight gradients of a backward stage in two launches (round 6).  A weight gradient has no consumer before the
 * optimizer (reference trainer.py:103-111: loss.backward() completes, then optimizer.step()), so the autograd nodes of
 * the host mirror only QUEUE their problem -- the nn.Linear weights of the unary blocks (models/blocks.py:481-515,
 * autograd's grad_out^T @ x) and the KPConv weights (blocks.py:369-374, with x := g / nn [Nq, Cout],
 * grad_out := weighted features [Nq, K Cin], grad_w viewed as [K Cin, Cout]) -- and the stage ends with ONE call:
 * one launch walks every problem's (row partition, output block) tasks, one more sums every problem's slabs in a fixed
 * order and finishes the queued bias gradients (as d3f_linear_grad_weight_bias).  Bit-reproducible, no atomics.
 * problems / n: HOST array.  grad_w [Cout, ldw]: row stride ldw >= Cin (a column block of a wider weight matrix is
 * written in place).  x, grad_out 16-byte aligned; Cin, Cout multiples of 16.  bias_part == NULL: no bias gradient. */
typedef struct d3f_atb_problem {
  const float* x;        /* [N, Cin] */
  const float* grad_out; /* [N, Cout] */
  float* grad_w;         /* [Cout, ldw] */
  int32_t N, Cin, Cout, ldw;
  const float* bias_part;
  int32_t bias_blocks, bias_cols;
  float* grad_bias;
  float* grad_bias2;
} d3f_atb_problem;
size_t d3f_linear_grad_weight_group_ws_bytes(const d3f_atb_problem* problems_host, int n);
int d3f_linear_grad_weight_group(const d3f_atb_problem* problems_host, int n, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pools -- replace models/blocks.py:94-110 (max_pool) and :79-91 (closest_pool).
 * ---------------------------------------------------------------------------------------------- */
/* out[n,c] = max_h x'[idx[n,h],c], x' = x plus a zero shadow row; argmax_out [Nq,C] int32 = winning support row
 * (Ns if the shadow won), saved for backward.
 * grad_x_clear (optional, [Ns,C]): the backward's scatter target, zeroed by the forward launch on the side; the backward
 * is then called with grad_x_precleared = 1 and launches no fill. */
/* width_dev (optional, device int32[1]): the table's max neighbor count as d3f_radius_query reports it; only the
 * first min(H, *width_dev) columns take part, which is the table the reference would have built
 * (dataloader.py:64-66 trims to the max count) when idx is kept at a wider, static width.
 * q_len (optional, [B]) + group: the batch stacks several reference batches (groups of `group` consecutive clouds, e.g.
 * 8 pairs); width_dev is then an array with one entry per group and every query row uses its own group's. */
int d3f_max_pool_forward(const float* x, int Ns, int C, const int32_t* idx, int Nq, int H, float* out,
                         int32_t* argmax_out, float* grad_x_clear, const int32_t* width_dev, const int32_t* q_len,
                         int B, int group, void* stream);
int d3f_max_pool_backward(const float* grad_out, const int32_t* argmax, int Nq, int C, int Ns, float* grad_x,
                          int grad_x_precleared, void* stream);
/* out[n,:] = x'[idx[n,0],:]  (idx has row stride H); backward: grad_out has row stride ld >= C (a column slice of
 * the gradient of the decoder's concatenation is consumed in place) */
/* skip (optional, [Nq, Cs]): out is [Nq, C + Cs] = [upsampled | skip], the decoder's torch.cat([x, skip], dim=1)
 * (models/architectures.py:311-313) done by the same launch; Cs = 0: plain closest_pool. */
int d3f_closest_pool_forward(const float* x, int Ns, int C, const int32_t* idx, int Nq, int H, const float* skip,
                             int Cs, float* out, float* grad_x_clear, void* stream);
int d3f_closest_pool_backward(const float* grad_out, int ld, const int32_t* idx, int Nq, int H, int C, int Ns,
                              float* grad_x, int grad_x_precleared, void* stream);
/* Gather forms for the deterministic mode: no float atomic, every row of grad_x [Ns,C] written once (no clearing), the
 * same bits on every call.  rev_ptr [Ns+1] / rev_ent = the CSR transpose d3f_reverse_table_build gives (queries per
 * support, ascending); every sum runs left to right in float32 over ascending query rows.
 * d3f_max_pool_backward_gather replaces the scatter of d3f_max_pool_backward: rev of the pooling table idx [Nq,H];
 *   grad_x[s,c] = grad_base[s,c] + sum of grad_out[q,c] over the q that list s with argmax[q,c] == s.  grad_base (optional,
 *   [Ns,C], may be grad_x itself): a gradient an older consumer left for the same tensor; it is the FIRST term.
 * d3f_closest_pool_backward_gather replaces the scatter of d3f_closest_pool_backward: rev of COLUMN 0 of the upsampling
 *   table as a [Nq,1] table; grad_x[s,c] = sum of grad_out[n*ld + c] over the n with idx[n,0] == s. */
int d3f_max_pool_backward_gather(const float* grad_out, const int32_t* argmax, int Nq, int C, int Ns,
                                 const int32_t* rev_ptr, const int32_t* rev_ent, const float* grad_base, float* grad_x,
                                 void* stream);
int d3f_closest_pool_backward_gather(const float* grad_out, int ld, int Nq, int C, int Ns, const int32_t* rev_ptr,
                                     const int32_t* rev_ent, float* grad_x, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Block epilogue -- replaces BatchNormBlock's bias add (models/blocks.py:473, use_bn=False), nn.LeakyReLU(0.1)
 *   (:497,:598,:676), the bottleneck's residual add (:686) and, in backward, PyTorch's bias-gradient reduction.
 *   out = act(x + bias1 + (add + bias2)), act(v) = v > 0 ? v : slope*v  (slope = 1: identity); bias1/add/bias2 optional.
 *   backward: grad_x = grad_out * (out > 0 ? 1 : slope)  (also the gradient of `add`);
 *             grad_bias[c] = sum_n grad_x[n,c]  (gradient of bias1 and bias2; OVERWRITTEN); grad_bias2 (optional)
 *             receives the same sums in a second buffer (two parameters, identical gradients).
 * zero_init (optional, zero_n floats): scratch the forward kernel clears on the side -- the backward's bias-gradient
 *   accumulators, so that backward (bias_prezeroed = 1) needs no separate fill launch.
 * row_div (optional, [N]): out = act(x[n,:]/row_div[n] + ...) and grad_x[n,:] = masked gradient / row_div[n] (the bias
 *   sums use the undivided masked gradient) -- the KPConv neighbor-count normalisation when x is a raw wf @ W product.
 * add_idx (optional, int32 with row stride idx_stride): `add` is then a COARSE matrix [add_rows, C] and row n receives
 *   add[add_idx[n*idx_stride]] (zeros for a shadow index) -- nearest upsampling folded into the epilogue.
 * ---------------------------------------------------------------------------------------------- */
int d3f_bias_act_forward(const float* x, const float* bias1, const float* add, const float* bias2, float slope, int N,
                         int C, float* out, float* zero_init, int zero_n, const float* row_div, const int32_t* add_idx,
                         int idx_stride, int add_rows, void* stream);
/* The same launch, additionally preparing the KPConv that consumes `out` as its input features: spack_out [N] float4 =
 * {s_pts[n], (sum_c out[n,c] > 0)} (the packed supports d3f_kpconv_forward would otherwise build with a launch of its
 * own) and zero_like_out (optional, [N,C]) cleared (that KPConv's grad_x scatter target).  C in {16,...,512} with C/4 a
 * power of two (d3f_bias_act_packs(C)). */
int d3f_bias_act_packs(int C);
int d3f_bias_act_forward_pack(const float* x, const float* bias1, const float* add, const float* bias2, float slope,
                              int N, int C, float* out, float* zero_init, int zero_n, const float* row_div,
                              const int32_t* add_idx, int idx_stride, int add_rows, const float* s_pts,
                              void* spack_out, float* zero_like_out, void* stream);
/* ws (optional, d3f_bias_act_backward_ws_bytes): with it, N >= 4096 uses per-block partial sums + a second tiny
 * launch for the bias gradient instead of atomics on C addresses (which serialise: 32 us at 38k x 32), deterministic. */
size_t d3f_bias_act_backward_ws_bytes(int N, int C);
int d3f_bias_act_backward(const float* grad_out, const float* out, float slope, int N, int C, float* grad_x,
                          float* grad_bias, float* grad_bias2, int bias_prezeroed, const float* row_div, void* ws,
                          size_t ws_bytes, void* stream);
/* The two passes of the many-row form separately (N >= 4096: d3f_bias_act_backward_blocks(N, C) > 0 partial rows):
 * _partial writes grad_x (optional) and the partial column sums ws [blocks, C]; the bias gradient is finished either by
 * d3f_linear_grad_weight_bias -- inside the launch that sums the weight gradient's slabs -- or by d3f_bias_sum. */
int d3f_bias_act_backward_blocks(int N, int C);
int d3f_bias_act_backward_partial(const float* grad_out, const float* out, float slope, int N, int C, float* grad_x,
                                  const float* row_div, void* ws, size_t ws_bytes, void* stream);
int d3f_bias_sum(const float* part, int blocks, int C, float* grad_bias, float* grad_bias2, void* stream);
/* The two-pass form at EVERY row count, for the deterministic mode: replaces the float atomics with which
 * d3f_bias_act_backward flushes its per-block column sums below 4096 rows.  The sums go to ws [blocks, C] and are added
 * up in block order; grad_bias / grad_bias2 are OVERWRITTEN.  ws >= d3f_bias_act_backward_ordered_ws_bytes(N, C). */
size_t d3f_bias_act_backward_ordered_ws_bytes(int N, int C);
int d3f_bias_act_backward_ordered(const float* grad_out, const float* out, float slope, int N, int C, float* grad_x,
                                  float* grad_bias, float* grad_bias2, const float* row_div, void* ws, size_t ws_bytes,
                                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * Deformable KPConv -- replaces the deformable=True branch of KPConv.forward (models/blocks.py:243-257,286-324,365-366).
 *   kp_def [Nq,K,3] = offsets * 1 + kernel_points, the per-query kernel points (offsets come from the rigid
 *   `offset_conv`, :190-199,244-254, which runs on d3f_kpconv_forward).  A neighbor is live when it is a real support
 *   AND within `extent` of at least one deformed kernel point (extent_sq = the float32 the reference compares against,
 *   (float)(KP_extent**2), :304); dead neighbors count neither for the weights nor for the neighbor number (:304-321).
 *   aggregate: wf [Nq,K*Cin] = sum_{h live} w_mode x[idx],  nn [Nq] = max(1, #live neighbors with a positive feature
 *              sum), min_d2 [Nq,K] = min_h d2[n,h,k] and min_idx [Nq,K] = the support attaining it (Ns when the row has
 *              no real neighbor; min_d2 is then the distance to the reference's shadow point at 1e6) -- both optional.
 *   grad:      from gwf = dL/dwf: grad_x [Ns,Cin] (OVERWRITTEN; optional) and grad_kp [Nq,K,3] (optional), the
 *              gradient w.r.t. the deformed kernel points through the influence weights.
 *   The caller applies the modulations, the contraction with the kernel weights and the division by nn.
 *   mode as d3f_kpconv_aggregate_modes.
 * ---------------------------------------------------------------------------------------------- */
int d3f_kpconv_deform_aggregate(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                                const float* x, int Cin, const float* kp_def, int K, float extent, float extent_sq,
                                int mode, float* wf_out, float* nn_out, float* min_d2_out, int32_t* min_idx_out,
                                void* stream);
int d3f_kpconv_deform_grad(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                           const float* x, int Cin, const float* kp_def, int K, float extent, float extent_sq, int mode,
                           const float* gwf, float* grad_x, float* grad_kp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batch normalisation over the stacked points -- replaces the use_bn=True branch of BatchNormBlock
 *   (models/blocks.py:454-455,465-471: nn.BatchNorm1d(C, momentum) over x [N, C] viewed as [1, C, N]).
 *   training != 0: y = (x - mean) / sqrt(var + eps) * gamma + beta with the batch mean and BIASED batch variance;
 *                  running_mean / running_var (optional) are updated in place: (1-m) old + m new, the variance
 *                  UNBIASED (N/(N-1)), like torch.
 *   training == 0: the running statistics normalise (both required).
 *   slope: LeakyReLU fused behind (1 = none).  gamma / beta may be NULL (1 / 0).  save_mean / save_invstd [C]
 *   (optional forward outputs) are what the backward needs.  n_live (optional int32 device scalar): only the first
 *   min(N, *n_live) rows are live -- N is then a capacity; dead rows are written as zeros.
 *   backward: grad_x (optional), grad_gamma, grad_beta (optional, OVERWRITTEN) for grad_y taken behind the activation.
 * Deterministic (fixed-order partial sums in ws).
 * ---------------------------------------------------------------------------------------------- */
size_t d3f_batchnorm_ws_bytes(int N, int C);
int d3f_batchnorm_forward(const float* x, int N, int C, const int32_t* n_live, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps, int training,
                          float slope, float* y, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                          void* stream);
int d3f_batchnorm_backward(const float* x, int N, int C, const int32_t* n_live, const float* gamma, const float* beta,
                           const float* save_mean, const float* save_invstd, float slope, int training,
                           const float* grad_y, float* grad_x, float* grad_gamma, float* grad_beta, void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Detector score -- replaces KPFCNN.detection_scores (models/architectures.py:322-368).
 * feat [N,C] un-normalised descriptors, idx = neighbors[0] [N,H].  feat_max [1] is a device scalar holding
 * max(feat) (d3f_global_max computes it).  training != 0: soft score; training == 0 additionally applies the
 * local-maximum gate (:361-366).
 * ---------------------------------------------------------------------------------------------- */
int d3f_global_max(const float* x, size_t n, float* out_max, void* ws /* >= 4 bytes */, size_t ws_bytes, void* stream);
/* same over the first sum(len) rows of x [cap_rows, C] (row count read on the device) */
int d3f_global_max_rows(const float* x, int cap_rows, int C, const int32_t* len, int B, float* out_max, void* ws,
                        size_t ws_bytes, void* stream);
/* one maximum per group of `group` consecutive clouds: out_max [ceil(B/group)] (ws >= 4 bytes per group).  The
 * reference normalises the detector features by the maximum of ITS batch (one pair, architectures.py:342); with 8
 * pairs stacked the normaliser has to stay per pair. */
int d3f_global_max_groups(const float* x, int cap_rows, int C, const int32_t* len, int B, int group, float* out_max,
                          void* ws, size_t ws_bytes, void* stream);
/* aux (optional, training only, [N, d3f_detection_scores_aux_floats(C)]): per-point scalars of the winning channel,
 * left behind so that the backward pass does not gather features again. */
int d3f_detection_scores_aux_floats(int C); /* 8 for C in {16, 32, 64}, 0 (aux unsupported) otherwise */
/* width (optional, device int32[1]): max neighbor count of the table when idx is kept wider than the reference would
 * build it (min(limit, max_count) columns, dataloader.py:64-66): the extra all-shadow columns are then ignored -- they
 * would give the eval-mode local-maximum gate a zero candidate the reference does not have.
 * len (optional, [B]) + group: stacked reference batches (see d3f_max_pool_forward): feat_max and width are arrays with
 * one entry per group (d3f_global_max_groups; d3f_radius_query_ex max_count_group). */
int d3f_detection_scores_forward(const float* feat, int N, int C, const int32_t* idx, int H, const float* feat_max,
                                 int training, float* scores, float* aux, const int32_t* width, const int32_t* len,
                                 int B, int group, void* stream);
/* grad_feat [N,C] is OVERWRITTEN.  Includes the gradient through the global max normaliser.  aux: the forward's
 * (optional; without it the neighborhood statistics are recomputed). */
int d3f_detection_scores_backward(const float* feat, int N, int C, const int32_t* idx, int H, const float* feat_max,
                                  const float* grad_scores, const float* aux, float* grad_feat, void* ws,
                                  size_t ws_bytes, void* stream);
/* the same for stacked reference batches (len [B] + group as in the forward; feat_max [ceil(B/group)]): the gradient
 * through the normaliser stays inside each group -- P fragment pairs stacked into one TRAINING batch keep the
 * per-pair maximum of architectures.py:342 and its arg-max gradient.  ws >= d3f_detection_scores_ws_bytes (per-block partial
 * sums of every group, added up in a fixed order: no float atomics in the normaliser's gradient).  A point whose incoming
 * gradient is exactly 0 -- all but the correspondences of the detector loss, utils/loss.py:140-158 -- contributes nothing and
 * is skipped. */
int d3f_detection_scores_backward_groups(const float* feat, int N, int C, const int32_t* idx, int H,
                                         const float* feat_max, const float* grad_scores, const float* aux,
                                         float* grad_feat, const int32_t* len, int B, int group, void* ws,
                                         size_t ws_bytes, void* stream);
size_t d3f_detection_scores_ws_bytes(int N, int C);

/* ------------------------------------------------------------------------------------------------
 * The training loss (trainer.py:90-98) in four stages, each one forward and one backward entry: select + normalise the
 * sampled rows, the detector on those rows, then circle + detector loss or contrastive + detector loss.
 *
 * The pair dimension.  Every entry takes `pairs`: the fragment pairs of one training batch (the reference trains on one
 * pair per step, datasets/dataloader.py:73; stacking P of them into one launch sequence is this build's batching).  M is
 * the number of sampled correspondences PER PAIR and every per-pair array below gains a leading pair dimension:
 * anchor/positive/out_a/out_p [pairs*M,C], scores sa/sp [pairs*M], neg_mask / dist_keypts / dists [pairs,M,M],
 * out_scalars [pairs,6], stats [pairs * d3f_circle_det_loss_stats_floats(M)], aux [2*pairs*M,8] (all anchors, then all
 * positives).  Every pair is its own M x M problem.  pairs <= 32 (2*pairs <= 64 clouds in the rows stages).
 *
 * The sampled rows (select + normalise, detector): idx_a / idx_p int64 [pairs*M], element m at idx[m * idx_stride]
 * (2 = the columns of a [pairs*M,2] correspondence table, idx_p = idx_a + 1, read in place).
 *   pair_len NULL: the rows are global rows of x; pairs must be 1; idx_p is offset by *p_offset (device int32: rows of
 *     the first cloud, trainer.py:91-94) when given.
 *   pair_len [2*pairs] (device int32, the level-0 stack lengths; clouds 2p, 2p+1 of the stack are pair p): the rows are
 *     local to the pair's own clouds, as the dataset yields them, and each column is offset by the start of its cloud.
 *     p_offset must be NULL.
 * pairs*M <= 2^24.  Rows outside [0, N) are clamped.
 * ---------------------------------------------------------------------------------------------- */

/* Select + normalise -- replaces F.normalize over all N descriptors (models/architectures.py:318) + the four index
 * selections of trainer.py:91-94 and their backward:
 *   out[m,:] = x[row[m],:] / max(||x[row[m],:]||, 1e-12),  s[m] = scores[row[m]].
 * backward: grad_x [N,C] and grad_scores [N] are ONE allocation of N*(C+1) floats (grad_scores == grad_x + N*C),
 * overwritten; g_* may be NULL.
 * scores NULL (forward; sa / sp are then not written) and grad_scores NULL (backward; only grad_x [N,C] is cleared and
 * written): the detector runs on the sampled rows itself (d3f_detection_rows_forward / _backward). */
int d3f_select_normalize_forward(const float* x, const float* scores, int N, int C, const int64_t* idx_a,
                                 const int64_t* idx_p, int idx_stride, int M, int pairs, const int32_t* p_offset,
                                 const int32_t* pair_len, float* out_a, float* out_p, float* sa, float* sp,
                                 void* stream);
int d3f_select_normalize_backward(const float* x, int N, int C, const int64_t* idx_a, const int64_t* idx_p,
                                  int idx_stride, int M, int pairs, const int32_t* p_offset, const int32_t* pair_len,
                                  const float* g_a, const float* g_p, const float* g_sa, const float* g_sp,
                                  float* grad_x, float* grad_scores, void* stream);

/* The detector on the SAMPLED rows: the loss reads the scores of the 2*pairs*M correspondences only (trainer.py:90-97
 * and :158-165 index scores[corr] before det_loss), so one wave per sampled row runs the body of
 * d3f_detection_scores_forward (the same device function: the scores are bit-identical to the dense ones) and leaves
 * sa, sp and a compact aux (NULL when no backward follows or training == 0).
 * feat_max / width / len [B] + group are the normaliser groups of d3f_detection_scores_forward (group 0: one normaliser
 * for the whole batch); with pair_len and len both given the groups are made of the pairs' clouds: B == 2*pairs.
 * C in {16, 32, 64} and H <= 64 (d3f_detection_rows_supported); anything else is D3F_EINVAL: the caller keeps the dense
 * path.
 * backward: g_sa / g_sp (either may be NULL = 0) are d loss / d sa, sp.  The gradient of x -- the three per-row terms
 * of d3f_detection_scores_backward and the normaliser's arg-max term -- is ADDED to grad_x [N,C] with float atomics:
 * grad_x is the buffer d3f_select_normalize_backward (grad_scores NULL) has just cleared and written its rows
 * into, so one fill serves both.  The arg-max positions are found by reading feat only; the normaliser's term is summed
 * from one partial per sampled row in a fixed order (the same bits on every replay).
 * ws >= d3f_detection_rows_ws_bytes(2*pairs*M). */
int d3f_detection_rows_supported(int C, int H);
size_t d3f_detection_rows_ws_bytes(int rows);
int d3f_detection_rows_forward(const float* feat, int N, int C, const int32_t* idx, int H, const float* feat_max,
                               int training, const int32_t* width, const int32_t* len, int B, int group,
                               const int64_t* idx_a, const int64_t* idx_p, int idx_stride, int M, int pairs,
                               const int32_t* p_offset, const int32_t* pair_len, float* sa, float* sp, float* aux,
                               void* stream);
int d3f_detection_rows_backward(const float* feat, int N, int C, const int32_t* idx, int H, const float* feat_max,
                                const int32_t* len, int B, int group, const int64_t* idx_a, const int64_t* idx_p,
                                int idx_stride, int M, int pairs, const int32_t* p_offset, const int32_t* pair_len,
                                const float* aux, const float* g_sa, const float* g_sp, float* grad_x, void* ws,
                                size_t ws_bytes, void* stream);
/* Order-fixed backward of the loss node's sampled rows, for the deterministic mode: replaces the float-atomic scatters of
 * d3f_select_normalize_backward (into grad_x and grad_scores) and of d3f_detection_rows_backward (c*, c', neighbor and
 * arg-max terms) into the one dense gradient.  Two entries with a key sort by the caller between them:
 *   _records  stores every contribution of sampled row m2 (anchors, then positives) as rec_key / rec_val
 *             [2*pairs*M, R], R = d3f_loss_rows_record_width(C, H) = C + 3 + H slots per row: slot c < C the
 *             normalisation's term of (row, c); C and C + 1 the detector's c* and c' terms; C + 2 + h the term of neighbor
 *             slot h; C + 2 + H the row's score gradient.  Record r = m2 * R + slot has rec_key = element * (rows * R) + r
 *             (element of grad_x, or N*C + row of grad_scores), INT64_MAX where the atomic forms add nothing.
 *             aux / idx / feat_max NULL and H = 0: no rows-form detector (g_sa / g_sp are then score gradients, kept with
 *             with_scores = 1).
 *   _apply    takes the keys SORTED ascending: clears grad_x [N, C] (+ [N] scores behind it with with_scores), gives every
 *             element the float32 sum of its records in key order -- ascending m2, inside a row normalise, c*, c',
 *             neighbors by slot -- and, with_detector, adds each group's arg-max term LAST.  tie_term_out (optional, one
 *             float per group) receives that term.
 * ws is the SAME buffer in both calls (>= d3f_detection_rows_ws_bytes(2*pairs*M)); rows = 2*pairs*M. */
int d3f_loss_rows_record_width(int C, int H);
int d3f_loss_rows_backward_records(const float* feat, int N, int C, const int32_t* idx, int H, const float* feat_max,
                                   const int32_t* len, int B, int group, const int64_t* idx_a, const int64_t* idx_p,
                                   int idx_stride, int M, int pairs, const int32_t* p_offset, const int32_t* pair_len,
                                   const float* aux, const float* g_a, const float* g_p, const float* g_sa,
                                   const float* g_sp, int with_scores, int64_t* rec_key, float* rec_val, void* ws,
                                   size_t ws_bytes, void* stream);
int d3f_loss_rows_backward_apply(const float* feat, int N, int C, int H, const float* feat_max, const int32_t* len, int B,
                                 int group, int rows, int with_detector, int with_scores, const int64_t* sorted_key,
                                 const float* rec_val, float* grad_x, float* tie_term_out, void* ws, size_t ws_bytes,
                                 void* stream);

/* Circle + detector loss -- replaces utils/loss.py: cdist(:8-44, 'euclidean'), CircleLoss.forward(:111-141),
 * DetLoss.forward(:149-158).  M in 2..1024 sampled correspondences.
 * anchor/positive [M,C]; neg_mask [M,M] uint8 = (dist_keypts > safe_radius), evaluated by the caller in the
 * dtype the dataset supplies (float64 in the reference, loss.py:116); anc_score/pos_score [M].
 * Outputs: dists [M,M], furthest_positive [M], average_negative [M],
 *   out_scalars[0..5] = desc_loss, det_loss, accuracy(%), mean furthest_positive, mean average_negative,
 *                      desc_loss + det_loss;
 *   out_total [1] (may be NULL) = sum_p (w_desc desc_p + w_det det_p): its gradient is the SUM of the pairs' gradients
 *                      (the caller's optimizer scale makes the mean);
 *   stats [d3f_circle_det_loss_stats_floats(M)] = row/column log-sum-exps + closest negatives, kept for backward.
 * backward: gradients of  sum_p (grad_desc w_desc desc_p + grad_det w_det det_p)  (grad_desc / grad_det device
 *   scalars; either may be NULL = 0; a caller that differentiates out_total passes its gradient as both)
 *   wrt anchor, positive and the two score vectors (optional).
 * Two routes.  M <= 128 and C <= 64 (the training and validation shapes): strips of every pair's matrix, one workgroup
 *   each, then one tiny launch for the scalars; backward one launch; ws is not used and may be NULL.
 *   Otherwise ONE workgroup works on the global buffers: pairs must be 1, w_desc = w_det = 1 and out_total NULL
 *   (D3F_EINVAL else), and the backward needs ws >= d3f_circle_det_loss_ws_bytes(M). */
size_t d3f_circle_det_loss_stats_floats(int M);
size_t d3f_circle_det_loss_ws_bytes(int M);
int d3f_circle_det_loss_forward(const float* anchor, const float* positive, int M, int C, int pairs,
                                const uint8_t* neg_mask, const float* anc_score, const float* pos_score, float log_scale,
                                float safe_radius, float pos_margin, float neg_margin, float w_desc, float w_det,
                                float* dists, float* furthest_positive, float* average_negative, float* out_scalars,
                                float* out_total, float* stats, void* stream);
int d3f_circle_det_loss_backward(const float* anchor, const float* positive, int M, int C, int pairs,
                                 const uint8_t* neg_mask, const float* anc_score, const float* pos_score, float log_scale,
                                 float safe_radius, float pos_margin, float neg_margin, float w_desc, float w_det,
                                 const float* dists, const float* stats, const float* grad_desc, const float* grad_det,
                                 float* grad_anchor, float* grad_positive, float* grad_anc_score, float* grad_pos_score,
                                 void* ws, size_t ws_bytes, void* stream);

/* Batch-hard contrastive loss + detector loss -- replaces utils/loss.py: ContrastiveLoss.forward(:54-62) with
 * metric 'euclidean' (what training_3DMatch.py:119-125 builds for desc_loss 'contrastive'), calculate_loss(:65-97) and
 * DetLoss.forward(:149-158) on its dists.  Two launches forward (one wave per row, then the scalars), one backward.
 *   dists = D + 10*near,  near_ij = (dist_keypts_ij + (i == j ? 10 : 0)) < safe_radius  (f64, like the reference's
 *   NumPy); furthest_positive = dists_ii, closest negative cn_i = min_{j != i} dists_ij (lowest j on ties);
 *   desc = mean_i [max(fp_i - pos_margin, 0) + max(neg_margin - cn_i, 0)], det = mean_i (fp_i - cn_i)(sa_i + sp_i).
 * anchor/positive [M,C] (C <= 256), dist_keypts [M,M] float64, scores [M]; M in 2..1024.  Outputs, out_scalars,
 * out_total, w_desc / w_det and grad_desc / grad_det as d3f_circle_det_loss_forward / _backward; stats
 * [d3f_circle_det_loss_stats_floats(M)] hold what the backward reads.  The gradients are those torch autograd forms:
 * half the gradient where a hinge is exactly 0. */
int d3f_contrastive_det_loss_forward(const float* anchor, const float* positive, int M, int C, int pairs,
                                     const double* dist_keypts, const float* anc_score, const float* pos_score,
                                     double safe_radius, float pos_margin, float neg_margin, float w_desc, float w_det,
                                     float* dists, float* furthest_positive, float* average_negative,
                                     float* out_scalars, float* out_total, float* stats, void* stream);
int d3f_contrastive_det_loss_backward(const float* anchor, const float* positive, int M, int C, int pairs,
                                      const float* anc_score, const float* pos_score, float pos_margin, float neg_margin,
                                      float w_desc, float w_det, const float* stats, const float* grad_desc,
                                      const float* grad_det, float* grad_anchor, float* grad_positive,
                                      float* grad_anc_score, float* grad_pos_score, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense matching -- replaces build_correspondence (geometric_registration/common.py:5-21): the
 * [Ns,Nt] distance matrix sqrt(2 - 2 S.T^T) is never materialised; ONE sweep of an f32 MFMA tile kernel over the
 * S x T tiles (the reference forms S T^T once, common.py:9) keeps a running row arg-min in registers and the column
 * arg-min of each workgroup's rows in LDS; the target range is split over workgroups and merged with one 64-bit
 * atomicMin per row / per column on (distance bits, index).  row_argmin [Ns], col_argmin [Nt] int32
 * (lowest index on ties, like np.argmin), mutual [Ns] int32 (optional) = 1 where col_argmin[row_argmin[i]] == i.
 * C in {16, 32, 64, 128}.
 * ---------------------------------------------------------------------------------------------- */
size_t d3f_mutual_nn_ws_bytes(int Ns, int Nt);
int d3f_mutual_nn(const float* src_desc, int Ns, const float* tgt_desc, int Nt, int C, int32_t* row_argmin,
                  int32_t* col_argmin, int32_t* mutual, void* ws, size_t ws_bytes, void* stream);
/* P independent matchings by ONE sweep launch (BASELINE configs[3]: 8 fragment pairs per inference batch).
 * seg [P,4] int32 ON THE DEVICE = {src_off, src_len, tgt_off, tgt_len} per pair: rows of src_desc / tgt_desc (which
 * may be the same stacked matrix).  max_src / max_tgt: host upper bounds of the lengths (they size the grid).
 * row_argmin [src_rows] / col_argmin [tgt_rows] / mutual [src_rows] are indexed by the row of the stacked matrix and
 * hold PAIR-LOCAL indices (what P separate d3f_mutual_nn calls return); rows outside every segment are untouched. */
size_t d3f_mutual_nn_batched_ws_bytes(int src_rows, int tgt_rows);
int d3f_mutual_nn_batched(const float* src_desc, int src_rows, const float* tgt_desc, int tgt_rows, const int32_t* seg,
                          int P, int max_src, int max_tgt, int C, int32_t* row_argmin, int32_t* col_argmin,
                          int32_t* mutual, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * k-nearest descriptor matching -- the k best target rows of every source row, for the estimators that take plain,
 * top-k or ratio-tested nearest neighbours instead of mutual ones.  csrc/knn_match.hpp has the rule: the distance is
 * the reference's sqrt(2 - 2 S T^T) in f32, correctly rounded; neighbours ascend by (distance, target index), a NaN
 * distance (2 - 2a < 0) first, like np.argmin; slot 0 is d3f_mutual_nn's row_argmin.  idx [Ns,k] int32, dist [Ns,k]
 * f32 (NaN where the reference's distance is); slots beyond Nt hold -1 / +inf.  1 <= k <= D3F_KNN_MAX, C in
 * {16, 32, 64, 128}.  The sweep of d3f_mutual_nn without its column side; a lane keeps its best k per row in
 * registers, the column chunks (d3f_tunables.match_wgs) meet in the workspace: two launches, no atomics, the same
 * result from run to run and for any chunking.
 * The batched form has d3f_mutual_nn_batched's conventions: seg [P,4], outputs indexed by stacked source row, PAIR-LOCAL
 * indices; the rows of a pair with an empty target get -1 / +inf, rows outside every segment are untouched.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_KNN_MAX 8
size_t d3f_knn_match_ws_bytes(int Ns, int Nt, int k);
int d3f_knn_match(const float* src_desc, int Ns, const float* tgt_desc, int Nt, int C, int k, int32_t* idx, float* dist,
                  void* ws, size_t ws_bytes, void* stream);
size_t d3f_knn_match_batched_ws_bytes(int src_rows, int P, int max_src, int max_tgt, int k);
int d3f_knn_match_batched(const float* src_desc, int src_rows, const float* tgt_desc, int tgt_rows, const int32_t* seg,
                          int P, int max_src, int max_tgt, int C, int k, int32_t* idx, float* dist, void* ws,
                          size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Keypoint selection -- replaces np.argsort(scores)[-k:] (test.py:56-57, geometric_registration/evaluate): the k
 * highest-scoring rows of every cloud of a stacked batch, in ascending (score, index) order like a stable argsort's
 * tail.  scores [rows]; seg [P,2] int32 on the device = {offset, length} per cloud; out [P,k] int32 CLOUD-LOCAL row
 * indices; a cloud with fewer than k rows fills its leading k - len slots with -1.  k <= D3F_TOPK_MAX.  One workgroup
 * per cloud: radix select of the k-th largest (score, index) key, then a rank sort of the survivors in LDS.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_TOPK_MAX 6144
int d3f_topk_scores(const float* scores, int rows, const int32_t* seg, int P, int k, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rigid registration -- replaces Open3D's registration_ransac_based_on_correspondence (3 points per hypothesis,
 * CorrespondenceCheckerBasedOnEdgeLength, inlier re-fits), which the reference leaves to Open3D on the CPU.
 * P correspondence sets in one stacked buffer: src / tgt [rows,3] f32 (row i of src matches row i of tgt); seg [P,2]
 * int32 ON THE DEVICE = (offset, count) per pair, like d3f_topk_scores.  Pair p is estimated from H hypotheses drawn by
 * the counter-based hash of (seed, first_pair + p, h, k) written in csrc/rigid.hpp (a batch split into chunks draws
 * what one call would when each chunk passes its first pair's index).  A hypothesis is invalid (never wins) when two
 * of its 3 indices are equal, either triangle is degenerate (|cross| < 1e-6) or, with edge_ratio > 0, an edge fails
 * min(la, lb) >= edge_ratio * max(la, lb).  Valid ones are fitted in f64 (Horn's quaternion form: always a proper
 * rotation) and score the correspondences with |R tgt + t - src|^2 < distance_threshold^2 in f32.  The winner has the
 * largest count, ties to the lowest h; it is refined refine_iters times (f64 least-squares fit over its inliers, fixed
 * summation order, then a recount).  Deterministic: integer counts, fixed-order f64 sums.  Two launches, no host
 * synchronisation (graph-capturable).
 * Outputs per pair: T [P,4,4] f64 mapping TARGET onto SOURCE (src ~ R tgt + t: the gt.log convention), inliers [P]
 * (final count), best_hypothesis [P] (winning h, -1 if none), best_count [P] (its count before refinement), status [P]
 * (D3F_RANSAC_ST_* bits; any bit set: T is the identity).  Optional (NULL to skip), for tests: hyp_count [P,H] int32
 * (-1 when invalid) and hyp_rt [P,H,12] f32 (R row-major, then t; zeros when invalid).
 * Limits: 1 <= H <= D3F_RANSAC_MAX_HYPOTHESES, count <= D3F_RANSAC_MAX_COUNT (a longer or out-of-range segment sets
 * D3F_RANSAC_ST_SEGMENT), 0 <= refine_iters <= D3F_RANSAC_MAX_REFINE, 0 <= edge_ratio <= 1, distance_threshold > 0,
 * P <= 65535; src / tgt may be NULL when rows = 0 (every pair then has fewer than 3 correspondences).
 * ---------------------------------------------------------------------------------------------- */
#define D3F_RANSAC_MAX_HYPOTHESES (1 << 24)
#define D3F_RANSAC_MAX_COUNT 65536
#define D3F_RANSAC_MAX_REFINE 64
#define D3F_RANSAC_ST_FEW 1           /* fewer than 3 correspondences */
#define D3F_RANSAC_ST_NO_HYPOTHESIS 2 /* no valid hypothesis among the H drawn */
#define D3F_RANSAC_ST_SEGMENT 4       /* segment outside [0, rows) or longer than D3F_RANSAC_MAX_COUNT */
size_t d3f_ransac_rigid_ws_bytes(int P, int H);
int d3f_ransac_rigid(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int first_pair, int H,
                     float distance_threshold, float edge_ratio, int refine_iters, uint64_t seed, double* T,
                     int32_t* inliers, int32_t* best_hypothesis, int32_t* best_count, int32_t* status,
                     int32_t* hyp_count, float* hyp_rt, void* ws, size_t ws_bytes, void* stream);
/* Host-only twins of the device code (csrc/rigid.hpp), for checking the sampler and solver without a GPU:
 * the 3 indices hypothesis h of pair p draws from count >= 1 correspondences; the least-squares rigid fit of n >= 1
 * pairs given as [n,3] f64 (src ~ R tgt + t) as a row-major 4x4. */
int d3f_ransac_sample_host(uint64_t seed, int p, int h, int count, int32_t* out_host);
int d3f_rigid_fit_host(const double* src_host, const double* tgt_host, int n, double* out_host);

/* ------------------------------------------------------------------------------------------------
 * Fast global registration -- replaces Open3D's registration_fgr_based_on_correspondence (Zhou, Park, Koltun, ECCV
 * 2016: tuple constraint, graduated non-convexity over a scaled Geman-McClure penalty), the RANSAC-free estimator the
 * reference's evaluation would hand the same correspondences to; like RANSAC the reference leaves it to Open3D on the
 * CPU.  Inputs and convention are d3f_ransac_rigid's: src / tgt [rows,3] f32, seg [P,2] int32 ON THE DEVICE =
 * (offset, count) per pair, T [P,4,4] f64 mapping TARGET onto SOURCE (src ~ R tgt + t).  The segments of different
 * pairs must not overlap (every row has one multiplicity slot).  The rule is written in full in csrc/fgr.hpp:
 *   tuple test   trial h of pair p draws 3 indices by the hash of (seed, first_pair + p, h, k) of csrc/rigid.hpp and
 *                passes when they are distinct, both triangles are non-degenerate and every edge satisfies
 *                min(la, lb) >= tuple_scale * max(la, lb); the first max_tuples passing trials in order of h (0: all)
 *                add 1 to the multiplicity m_i of their correspondences.  tuple_trials < 0: min(100 count,
 *                D3F_FGR_MAX_TRIALS) trials (Open3D's rule); 0: no test, every m_i = 1.
 *   objective    sum_i m_i rho_mu(|a_i - T b_i|), minimised by `iterations` line-process / Gauss-Newton steps on SE(3)
 *                about the centroids of the live (m_i > 0) rows, mu annealed from the squared extent of the pair to
 *                distance_threshold^2: divided by division_factor before every anneal_every-th iteration and clamped
 *                there.  mu is a squared distance in metres; there is no scene rescaling and no early exit.
 * One launch of P workgroups, f64 sums in a fixed order, no floating-point atomic, no host synchronisation
 * (graph-capturable); a pair's outputs are the same bits alone (with first_pair = its index) or in any batch.
 * Outputs per pair: T; inliers [P] = correspondences (all of them, whatever m_i) within distance_threshold under the
 * f32 image of T, the count d3f_ransac_rigid reports; tuples [P] = counted triples; weight_sum [P] f64 = sum of the
 * line-process weights of the last iteration; status [P] (D3F_FGR_ST_* bits; FEW, SEGMENT or NONFINITE: T is the
 * identity and inliers 0; SINGULAR: the pose of the iterations before stays).  Optional (NULL to skip), for tests:
 * multiplicity [rows] int32 (rows of no segment are not written) and trace [P, iterations, 8] f64 = (mu, weight_sum,
 * omega (3), v (3)) per iteration (iterations that did not run are not written).
 * Workspace: d3f_fgr_rigid_ws_bytes(rows) -- the multiplicities, 4 bytes per row.
 * Limits: 1 <= P <= D3F_FGR_MAX_PAIRS, 1 <= iterations <= D3F_FGR_MAX_ITERS, anneal_every >= 1, division_factor > 1,
 * 0 < tuple_scale <= 1, tuple_trials <= D3F_FGR_MAX_TRIALS, max_tuples >= 0, distance_threshold > 0, count <=
 * D3F_RANSAC_MAX_COUNT (a longer or out-of-range segment sets D3F_FGR_ST_SEGMENT); src / tgt may be NULL when rows = 0.
 * d3f_fgr_rigid_host: the host twin -- the same rule (csrc/fgr.hpp) on one CPU thread with the same summation order;
 * every pointer is a host pointer, no workspace, no GPU call.  It differs from the device only where the device's
 * sin / cos differ from the host's.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_FGR_MAX_PAIRS (1 << 20)
#define D3F_FGR_MAX_ITERS 1024
#define D3F_FGR_MAX_TRIALS (1 << 22)
#define D3F_FGR_ST_FEW 1        /* fewer than 3 correspondences, or fewer than 3 left by the tuple test */
#define D3F_FGR_ST_SINGULAR 2   /* the 6x6 system lost a pivot: the pair stopped at the pose it had */
#define D3F_FGR_ST_SEGMENT 4    /* segment outside [0, rows) or longer than D3F_RANSAC_MAX_COUNT */
#define D3F_FGR_ST_NONFINITE 8  /* a coordinate or a sum is not finite */
size_t d3f_fgr_rigid_ws_bytes(int rows);
int d3f_fgr_rigid(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int first_pair,
                  double distance_threshold, int iterations, double division_factor, int anneal_every,
                  double tuple_scale, int tuple_trials, int max_tuples, uint64_t seed, double* T, int32_t* inliers,
                  int32_t* tuples, double* weight_sum, int32_t* status, int32_t* multiplicity, double* trace, void* ws,
                  size_t ws_bytes, void* stream);
int d3f_fgr_rigid_host(const float* src_host, const float* tgt_host, int rows, const int32_t* seg_host, int P,
                       int first_pair, double distance_threshold, int iterations, double division_factor,
                       int anneal_every, double tuple_scale, int tuple_trials, int max_tuples, uint64_t seed,
                       double* T_host, int32_t* inliers_host, int32_t* tuples_host, double* weight_sum_host,
                       int32_t* status_host, int32_t* multiplicity_host, double* trace_host);

/* ------------------------------------------------------------------------------------------------
 * Spatial-compatibility pose estimation (second order; after SC^2-PCR, Chen et al., CVPR 2022) -- the estimator for
 * correspondence sets with a few per cent of inliers, without sampling and without a seed.  Inputs and convention are
 * d3f_ransac_rigid's: src / tgt [rows,3] f32, seg [P,2] int32 ON THE DEVICE = (offset, count) per pair (the segments do
 * not overlap), T [P,4,4] f64 mapping TARGET onto SOURCE (src ~ R tgt + t).  The rule is written in full in
 * csrc/sc2.hpp; with a_i / b_i the pair's source / target row i as exact f64 images and n its count:
 *   compatibility  i != j: A = |a_i - a_j|^2, B = |b_i - b_j|^2 summed as ((dx dx + dy dy) + dz dz), s = (A + B) -
 *                  compat_threshold^2, C_ij = (s < 0) || (s s < 4 (A B)); C_ii = 0.  No square root, no libm: the bits
 *                  are the same on device, host and in NumPy.  A non-finite coordinate leaves its row and column empty.
 *   seeds          degree d_i = popcount(row i); seed rank = rows by descending d_i, ties to the lower i; the first
 *                  min(num_seeds, n) ranks are seeds; a seed with d_i < 2 gives no hypothesis.
 *   consensus set  seed i, then the min(set_size - 1, d_i) rows j with C_ij = 1 by descending s_ij = popcount(row_i &
 *                  row_j), ties to the lower j, in that order.
 *   hypothesis     the f64 Horn fit (csrc/rigid.hpp) over the set in that order; its f32 image is scored over ALL n
 *                  rows as d3f_ransac_rigid scores, at (float)distance_threshold squared in f32.
 *   winner         the largest count, ties to the lowest seed rank; then d3f_ransac_rigid's refinement, refine_iters
 *                  times (csrc/rigid_refine.hpp), and a final recount.
 * Differences from the paper: seeds come from the integer degree (the paper: leading eigenvector and non-maximum
 * suppression); one selection stage and an unweighted fit (the paper: two stages, spectral weights); no sampling
 * anywhere; the authors' code was not at hand to compare with.
 * Four launches of static shape, no atomics, no host synchronisation (graph-capturable); a pair's outputs are the same
 * bits alone or in any batch.
 * Outputs per pair: T; inliers [P] (final count); best_seed [P] (the winning seed's row inside the pair, -1 if none);
 * best_count [P] (its count before refinement); status [P] (D3F_SC2_ST_* bits; any bit set: T is the identity and
 * inliers 0).  Optional (NULL to skip), for tests: degree [rows] int32 (rows of no segment are not written); seed_rows
 * [P,num_seeds] (the row of each rank, -1 beyond min(num_seeds, n)); consensus [P,num_seeds,set_size] (rows in set
 * order, -1 padded; written for every seed, also one with d_i < 2); hyp_count [P,num_seeds] (-1 when there is no
 * hypothesis); hyp_rt [P,num_seeds,12] f32 (R row-major, then t; zeros when there is no hypothesis).
 * Workspace: d3f_sc2_rigid_ws_bytes(P, max_count, num_seeds), five parts, each aligned to 256 bytes, in this order:
 *   bit matrix  uint64 [P, max_count, W], W = ceil(max_count / 64): pair p's matrix at word p * max_count * W, row i
 *               at i * W, bit l of word w = column 64 w + l; rows and bits >= n are 0;
 *   degrees     int32 [P, max_count];   seed table  int32 [P, num_seeds];
 *   keys        uint64 [P, num_seeds] = ((count + 1) << 32) | ~rank, 0 without a hypothesis;
 *   poses       f64 [P, num_seeds, 12] (written where there is a hypothesis).
 * The workspace need NOT be cleared by the caller: every word a launch reads was written by an earlier launch of the
 * same call.  The matrix is max_count * W * 8 bytes per pair: 3.2 MB at 5000.
 * Limits: 1 <= max_count <= D3F_SC2_MAX_COUNT, 3 <= set_size <= D3F_SC2_MAX_SET, 1 <= num_seeds <= D3F_SC2_MAX_SEEDS,
 * 1 <= P <= 65535, 0 <= refine_iters <= D3F_RANSAC_MAX_REFINE, both thresholds positive and finite; a segment out of
 * range or with count > max_count sets D3F_SC2_ST_SEGMENT; src / tgt may be NULL when rows = 0.
 * d3f_sc2_rigid_host: the host twin -- the same rule on one CPU thread, the same summation order in the refinement;
 * every pointer is a host pointer, no workspace, no GPU call.  In place of the workspace it takes matrix_host, optional
 * (NULL to skip): uint64 [P, max_count, W], the bit matrices.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_SC2_MAX_COUNT 8192
#define D3F_SC2_MAX_SET 64
#define D3F_SC2_MAX_SEEDS 4096
#define D3F_SC2_ST_FEW 1           /* fewer than 3 correspondences */
#define D3F_SC2_ST_NO_HYPOTHESIS 2 /* no seed has two compatible correspondences */
#define D3F_SC2_ST_SEGMENT 4       /* segment outside [0, rows) or longer than max_count */
size_t d3f_sc2_rigid_ws_bytes(int P, int max_count, int num_seeds);
int d3f_sc2_rigid(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int max_count,
                  double distance_threshold, double compat_threshold, int num_seeds, int set_size, int refine_iters,
                  double* T, int32_t* inliers, int32_t* best_seed, int32_t* best_count, int32_t* status, int32_t* degree,
                  int32_t* seed_rows, int32_t* consensus, int32_t* hyp_count, float* hyp_rt, void* ws, size_t ws_bytes,
                  void* stream);
int d3f_sc2_rigid_host(const float* src_host, const float* tgt_host, int rows, const int32_t* seg_host, int P,
                       int max_count, double distance_threshold, double compat_threshold, int num_seeds, int set_size,
                       int refine_iters, double* T_host, int32_t* inliers_host, int32_t* best_seed_host,
                       int32_t* best_count_host, int32_t* status_host, int32_t* degree_host, int32_t* seed_rows_host,
                       int32_t* consensus_host, int32_t* hyp_count_host, float* hyp_rt_host, uint64_t* matrix_host);

/* ------------------------------------------------------------------------------------------------
 * Training items from a device-resident 3DMatch split -- replaces the per-item host work of the reference's
 * ThreeDMatchDataset.__getitem__ (ThreeDMatch.py:93-149: float64 copies, rotation, two noise draws, a choice over the
 * correspondences, cdist) and the upload that follows it.  The split is stored once on the device as `points`
 * [sumN,3] f32 (all fragments packed) and `corr` [sumM,2] int32 (all pairs' tables packed, rows = fragment-local
 * (source, target) indices).  A job names one item: where its two clouds and its table sit in the stores, the rigid
 * transform of the target (R row-major 3x3, t; f64), a 64-bit item key and its four output buffers ON THE DEVICE:
 *   out_src [src_len,3] f32, out_tgt [tgt_len,3] f32, out_corr [m,2] int64, out_dist [m,m] f64,  m = min(corr_len, k).
 * All randomness is the counter-based hash of (key, stream, index) written in csrc/augment.hpp, which also fixes the
 * f64 operation order of the points and of out_dist; a job's outputs are the same bits alone or in any batch.
 * out_corr: corr_len > k: the k rows j with the smallest z(7, j), in ascending z (keys are distinct: no tie rule);
 * otherwise all rows in table order.  out_dist: distances between the augmented f32 source points of out_corr's rows.
 * d3f_augment_pairs: 1 <= B <= D3F_AUGMENT_MAX_JOBS jobs given as a HOST array that travels in the kernel argument;
 * two launches, no copy, no host synchronisation (graph-capturable).  The selection runs in one workgroup per job:
 * radix histograms of the recomputed keys in LDS narrow the k-th smallest down to at most D3F_AUGMENT_CANDIDATES
 * candidates, which are sorted in LDS; exact for every corr_len < 2^31, no global atomics.  It needs no global
 * workspace today: d3f_augment_pairs_ws_bytes(B, k) is 0 and ws may be NULL (callers still ask, so a later version can
 * take scratch).  1 <= k <= D3F_AUGMENT_MAX_NODE, noise >= 0 and finite, every corr_len >= 1, segments inside the
 * stores; a source index outside its cloud is clamped for the distance matrix (validate tables once on the host).
 * d3f_augment_item_host: the same for ONE job on HOST pointers (stores and outputs), from the same functions of
 * csrc/augment.hpp; returns m, or -1.  d3f_augment_key_host: z(stream, index) of item key `key`
 * (d3f_augment_key_host(0, 0, 0) = splitmix64(0) = 0xE220A8397B1DCDAF).
 * ---------------------------------------------------------------------------------------------- */
#define D3F_AUGMENT_MAX_JOBS 16
#define D3F_AUGMENT_MAX_NODE 1024
#define D3F_AUGMENT_CANDIDATES 1024
typedef struct d3f_augment_job {
  int64_t src_off, tgt_off; /* first row of the source / target cloud in `points` */
  int64_t corr_off;         /* first row of the pair's table in `corr` */
  int32_t src_len, tgt_len, corr_len, reserved;
  double R[9], t[3];
  uint64_t key;
  float* out_src;
  float* out_tgt;
  int64_t* out_corr;
  double* out_dist;
} d3f_augment_job;
size_t d3f_augment_pairs_ws_bytes(int B, int k);
int d3f_augment_pairs(const float* points, int64_t sum_n, const int32_t* corr, int64_t sum_m, const d3f_augment_job* jobs,
                      int B, int k, double noise, void* ws, size_t ws_bytes, void* stream);
int d3f_augment_item_host(const float* points_host, const int32_t* corr_host, const d3f_augment_job* job, int k,
                          double noise);
uint64_t d3f_augment_key_host(uint64_t key, int stream, uint32_t index);

/* ------------------------------------------------------------------------------------------------
 * Nearest neighbour within a radius over a list of cloud pairs -- the mining step of the 3DMatch training pickles
 * (datasets/preprocess.py; the reference ships the finished files and has no counterpart).
 * `points` [Ns,3] f32 are B clouds stacked, each in its OWN frame; cloud_start [B+1] int32 ON THE DEVICE is the prefix
 * of their lengths (cloud_start[0] = 0, cloud_start[B] live rows <= Ns).  d3f_cloud_grid_build makes ONE cell list over
 * all of them (workspace: d3f_radius_grid_ws_bytes(Ns)) with the cloud index as the batch element of the cell key,
 * B <= 65535.  It keeps the buckets and the stored points of every cloud contiguous (the searches against one target
 * stay inside ~40 B per target point), so it serves d3f_nearest_pairs only; d3f_nearest_pairs also takes a list that
 * d3f_radius_grid_build made over the same stack (B <= 64) -- the list records which of the two it is.
 * d3f_nearest_pairs: pair p = (pairs[2p] source cloud, pairs[2p+1] target cloud; equal is legal) with transforms[12p..]
 * a row-major 3x4 f64 matrix that maps source points into the target's frame.  Query row row_start[p] + i is point i of
 * the source cloud; row_start [P+1] int64 on the device is the prefix of the source lengths.  `rows` is the capacity of
 * out_nn (the launch is sized by it); rows beyond row_start[P] are left untouched.
 *   q  = f32(((T0 x + T1 y) + T2 z) + T3) per component, evaluated in f64 without contraction;
 *   d2 = ((dx dx) + (dy dy)) + (dz dz) in f32 without FMA, accepted when d2 < radius * radius (f32 product, strict);
 *   out_nn[row] = index INSIDE the target cloud of the accepted point with the least d2, the lowest index among equal
 *   d2, or -1; out_count[p] (caller-cleared) += rows of pair p that found one.
 * radius <= grid_radius (the radius the list was built with).  A query whose cell falls outside the addressable grid
 * sets D3F_ST_CELL_RANGE and yields -1; a pair that names a cloud outside [0, B), or a row beyond its source cloud,
 * yields -1.  One launch on `stream`, no host synchronisation, no allocation; integer results, identical from run to
 * run.  d3f_nearest_pairs_lanes is the same with the lanes that share one query chosen by the caller (4, 8, 16, 32;
 * 0 = the default, 8) -- for measurements; the result does not depend on it.
 * ---------------------------------------------------------------------------------------------- */
int d3f_cloud_grid_build(const float* points, int Ns, const int32_t* cloud_start, int B, float radius, void* grid_ws,
                         size_t grid_ws_bytes, int32_t* status, void* stream);
int d3f_nearest_pairs(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                      float grid_radius, float radius, const int32_t* pairs, const double* transforms,
                      const int64_t* row_start, int P, int64_t rows, int32_t* out_nn, int32_t* out_count,
                      int32_t* status, void* stream);
int d3f_nearest_pairs_lanes(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                            float grid_radius, float radius, const int32_t* pairs, const double* transforms,
                            const int64_t* row_start, int P, int64_t rows, int32_t* out_nn, int32_t* out_count,
                            int32_t* status, int lanes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point-to-point ICP over a list of cloud pairs -- the refinement every 3DMatch registration pipeline runs after RANSAC
 * (Open3D's registration_icp; the reference leaves it to Open3D on the CPU).  The clouds, the cell list (grid_ws,
 * grid_radius), cloud_start, pairs and row_start are those of d3f_nearest_pairs: pair p = (pairs[2p] MOVING cloud a,
 * pairs[2p+1] FIXED cloud b) and its transform maps points of a into b's frame.  For a gt.log key i_j, whose matrix
 * maps fragment j into fragment i (what d3f_ransac_rigid returns: "target onto source"), the moving cloud is j and the
 * fixed cloud is i: a RANSAC result is a valid T_init as it stands with pairs = (j, i).
 * T_init [P,12] f64: row-major 3x4 per pair.  All P pairs advance together; iteration k = 0, 1, ... of pair p:
 *   1. search under T_k with the arithmetic, acceptance (d2 < max_distance * max_distance, f32) and tie rule of
 *      d3f_nearest_pairs, and over the accepted rows, in f64: n, sum x', sum y', sum x' y'^T, sum d2 (the f32 d2
 *      widened); x' = x - px with x the ORIGINAL moving point and px row 0 of the moving cloud, y' = y - py with y the
 *      matched fixed point and py row 0 of the fixed cloud.  No index table is written.
 *   2. fitness_k = n / len(a), rmse_k = sqrt(sum d2 / n) (0 when n = 0).
 *      n < 3: stop, status D3F_ICP_ST_FEW.
 *      k >= 1 and |fitness_k - fitness_{k-1}| < rel_fitness and |rmse_k - rmse_{k-1}| < rel_rmse: stop (Open3D's
 *      ICPConvergenceCriteria, which compares absolute differences despite the names).
 *      k == max_iters: stop.
 *      else T_{k+1} = the least-squares fit y ~ R x + t from the sums (csrc/rigid.hpp fit_from_sums), next iteration.
 *   A stopped pair's result is T_k; max_iters = 0 only evaluates T_init.  At most max_iters + 1 searches.
 * Outputs per pair: T [P,4,4] f64; count [P] int32 and rmse [P] f64 of the RETURNED T (n_k, rmse_k of the stopping
 * iteration); iterations [P] int32 (fits applied); status [P] int32 (D3F_ICP_ST_* bits).  A pair that names a cloud
 * outside [0, B), or whose rows reach beyond `rows`, gets D3F_ICP_ST_PAIR; a non-finite T_init D3F_ICP_ST_NONFINITE;
 * both return T_init, count 0, rmse 0, iterations 0.  Optional (NULL to skip), for tests: trace [P, max_iters+1, 2] f64
 * = (n_k, sum d2_k) per search, NaN beyond the stop.
 * Deterministic and batch-independent: a workgroup serves D3F_ICP_BLOCK_ROWS consecutive rows of ONE pair, sums them
 * in a fixed tree, and the pair's workgroups are added in a fixed order that depends on the pair's length alone -- no
 * floating-point atomics -- so a pair's result is bit-identical alone or inside any batch and from run to run.
 * `rows` >= row_start[P] sizes the launches and the workspace (d3f_icp_rigid_ws_bytes(P, rows)); P <= 65535,
 * 0 <= max_iters <= D3F_ICP_MAX_ITERS, max_distance <= grid_radius.  1 + 2 (max_iters + 1) launches on `stream`
 * whatever the data, no host synchronisation, no allocation (graph-capturable).
 * d3f_icp_fit_host: host-only twin of step 2's fit: sums[17] = {n, sum x' (3), sum y' (3), sum x'_a y'_b (9), sum d2},
 * pivots px, py -> row-major 4x4; n >= 1.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_ICP_MAX_ITERS 1024
#define D3F_ICP_BLOCK_ROWS 512
#define D3F_ICP_ST_FEW 1        /* fewer than 3 accepted rows at the stopping iteration */
#define D3F_ICP_ST_CELL_RANGE 2 /* a moved point fell outside the addressable cell grid (= D3F_ST_CELL_RANGE) */
#define D3F_ICP_ST_PAIR 4       /* the pair names a cloud outside [0, B) or rows beyond `rows` */
#define D3F_ICP_ST_NONFINITE 8  /* T_init holds a non-finite value */
size_t d3f_icp_rigid_ws_bytes(int P, int64_t rows);
int d3f_icp_rigid(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                  float grid_radius, float max_distance, const int32_t* pairs, const int64_t* row_start, int P,
                  int64_t rows, const double* T_init, int max_iters, double rel_fitness, double rel_rmse, double* T,
                  int32_t* count, double* rmse, int32_t* iterations, int32_t* status, double* trace, void* ws,
                  size_t ws_bytes, void* stream);
int d3f_icp_fit_host(const double* sums_host, const double* px_host, const double* py_host, double* out_host);

/* ------------------------------------------------------------------------------------------------
 * Surface normals of every point of the stacked clouds of a cell list, and point-to-plane ICP with them.  The reference
 * leaves both to Open3D on the CPU (estimate_normals, TransformationEstimationPointToPlane).
 *
 * d3f_estimate_normals.  The cell list (grid_ws, grid_radius), points, Ns, cloud_start and B are those of
 * d3f_nearest_pairs; radius <= grid_radius; min_neighbors >= 1; viewpoint_host: 3 floats ON THE HOST, the same point in
 * every cloud's own frame, NULL for the origin.  The fill order of a bucket is decided by atomics, so the result is made
 * independent of the order in which neighbours are met BY CONSTRUCTION:
 *   neighbours of point i: the points j of the SAME cloud, i itself included, with
 *        d2 = ((dx dx) + (dy dy)) + (dz dz) < radius * radius   (f32 without FMA, f32 product, strict: the rule of the
 *        other searches; the cell key carries the cloud index, so clouds that overlap in coordinates never mix);
 *   Q  = 2^floor(log2(2^20 / radius)), computed on the host in double;
 *   u  = (int64) rint((double)(p_j - p_i) Q) per component, p_j - p_i ONE f32 subtraction, ties to even; |u| <= 2^20;
 *   moments (int64): n, sum u_x, sum u_y, sum u_z, sum u_x u_x, u_x u_y, u_x u_z, u_y u_y, u_y u_z, u_z u_z -- integer
 *        addition commutes, so lanes, groups and bucket order cannot change them (products < 2^40: 2^22 neighbours fit);
 *   C  = (S - s s^T / n) / n in f64; the normal is the unit eigenvector of C's smallest eigenvalue in f64 (cyclic
 *        Jacobi, a fixed number of sweeps; csrc/plane.hpp), rounded to f32;
 *   sign: n . (viewpoint - p_i) >= 0 (f64); when that is exactly 0 the first non-zero component is positive;
 *   n < min_neighbors, or a largest eigenvalue that is not positive: the normal is (0, 0, 0).
 * Outputs in input row order: normals [Ns,3] f32, count [Ns] int32 (= n), optional (NULL to skip) moments [Ns,10] int64.
 * Rows beyond cloud_start[B] get zeros.  A point outside the addressable cell grid is in no cell list: it has count 0
 * and sets D3F_ST_CELL_RANGE in *status.  One launch on `stream`, no host synchronisation, no allocation.
 * d3f_normal_from_moments_host: host-only twin of everything after the moments (the same inline code): m[10], Q and
 * to_view = viewpoint - p_i -> out[3]; n < 1 gives zeros (min_neighbors is the caller's test).
 *
 * d3f_icp_rigid_plane: d3f_icp_rigid with `normals` [Ns,3] f32 in input row order (the normals of the FIXED cloud are
 * used).  Setup, search, n_k, sum d2, fitness, rmse (Open3D's inlier_rmse is the point distance under every estimation
 * method), the stopping rule, count, rmse, trace and the reduction orders are those of d3f_icp_rigid.  Per accepted
 * row, in f64, with nrm the normal of the matched fixed point y and py row 0 of the fixed cloud:
 *   a = (((T0 x + T1 y) + T2 z) + T3) - py per component (T_k x in f64, NOT the f32 query), c = y - py,
 *   J = [a x nrm, nrm] (6), r = (a - c) . nrm;
 *   sums[29] = { n, the 21 upper entries of sum J J^T row by row, sum J r (6), sum d2 }.
 * Fit: Cholesky of the 6x6 in f64.  A pivot <= 1e-10 max_i A_ii stops the pair at its current pose with
 * D3F_ICP_ST_SINGULAR (the free slide of a single plane, or an overlap of zero normals).  Otherwise
 *   v = -A^-1 sum J r = (alpha, beta, gamma, t_d); R_d = Rz(gamma) Ry(beta) Rx(alpha) (Open3D's
 *   TransformVector6dToMatrix4d); R_{k+1} = R_d R_k; t_{k+1} = R_d (t_k - py) + py + t_d.
 * A zero normal contributes zeros to the fit and still counts in n_k.  Workspace: d3f_icp_rigid_plane_ws_bytes(P, rows).
 * d3f_icp_plane_fit_host: host-only twin of the fit: sums[29], py[3], T_k [12] (row-major 3x4) -> T_next [16]
 * (row-major 4x4; T_k when singular), *singular = 0 / 1.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_ICP_ST_SINGULAR 16  /* point-to-plane: the 6x6 normal equations are singular at the stopping iteration */
int d3f_estimate_normals(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                         float grid_radius, float radius, int min_neighbors, const float* viewpoint_host,
                         float* normals, int32_t* count, int64_t* moments, int32_t* status, void* stream);
int d3f_normal_from_moments_host(const int64_t* m_host, double Q, const double* to_view_host, float* out_host);
size_t d3f_icp_rigid_plane_ws_bytes(int P, int64_t rows);
int d3f_icp_rigid_plane(const void* grid_ws, const float* points, const float* normals, int Ns,
                        const int32_t* cloud_start, int B, float grid_radius, float max_distance, const int32_t* pairs,
                        const int64_t* row_start, int P, int64_t rows, const double* T_init, int max_iters,
                        double rel_fitness, double rel_rmse, double* T, int32_t* count, double* rmse,
                        int32_t* iterations, int32_t* status, double* trace, void* ws, size_t ws_bytes, void* stream);
int d3f_icp_plane_fit_host(const double* sums_host, const double* py_host, const double* T_k_host, double* T_next_host,
                           int* singular_host);

/* ------------------------------------------------------------------------------------------------
 * Coloured ICP: point-to-plane ICP with a colour term, so that a pair whose overlap is mostly one plane -- where the
 * point-to-plane residual leaves the slide along the plane free -- is held by the texture on that plane (Park, Zhou,
 * Koltun 2017; Open3D's registration_colored_icp).  csrc/color_icp.hpp states the rule beside the code.
 *
 * Intensity: one f32 per point in input row order beside the points.  It is USABLE when 0 <= I <= 1 compared as floats;
 * any other value, NaN included, means "no colour".  q = (int64) rint((double) I * 2^20).
 *
 * d3f_color_gradients.  The cell list (grid_ws, grid_radius), points, Ns, cloud_start, B, radius and the neighbourhood
 * are those of d3f_estimate_normals: the points j of the SAME cloud, i itself included, with d2 < radius * radius (f32,
 * strict), the same Q and u = rint((p_j - p_i) Q).  `normals` [Ns,3] f32 (the normal of the query row is read) and
 * `intensity` [Ns] f32 are inputs.  Only neighbours with a usable intensity count; a point whose OWN intensity is not
 * usable is not searched (count 0, zero moments).
 *   moments (int64) [13]: n, sum u (3), sum u u^T (xx xy xz yy yz zz) as for the normals, then sum u_x c, sum u_y c,
 *        sum u_z c with c = q_j - q_i; |u| <= 2^20 and |c| <= 2^20, a product is below 2^40 and 2^22 neighbours fit.
 *        All 13 are integers: lanes, groups, bucket order, stacking and cell size cannot change them.
 *   Everything after the moments is a function of them and of the f32 normal nrm of the row, in f64:
 *        S = sum u u^T / Q^2 (about the point, not centred); h = sum u c / (Q 2^20);
 *        e1 = normalise(nrm x axis), axis the unit vector of the component of nrm with the smallest magnitude (lowest
 *        index on ties); e2 = nrm x e1; E = [e1 e2]; G = E^T S E (2x2), g2 = E^T h;
 *        d = E G^-1 g2 by the closed form of the 2x2 (so d . nrm = 0 to rounding), rounded to f32: the least-squares
 *        slope of the intensity over the neighbourhood on the tangent plane, in intensity per unit length.
 *   invalid: the point's own intensity is not usable, n < min_neighbors (>= 1; 4 is the front ends' default), nrm is
 *        zero or not finite, or det G <= 1e-6 max(G00, G11)^2 (neighbours on one line).
 * Outputs in input row order: field [Ns,4] f32 = (d_x, d_y, d_z, I), 16-byte aligned; an invalid gradient is three
 * NaNs, an unusable intensity a NaN in .w.  Optional (NULL to skip): count [Ns] int32 (= n), moments [Ns,13] int64.
 * Rows beyond cloud_start[B] get four NaNs, count 0 and zero moments.  A point outside the addressable cell grid is in
 * no cell list: count 0, D3F_ST_CELL_RANGE in *status.  One launch on `stream`, no host synchronisation, no
 * allocation, no LDS, no floating-point atomics.
 * d3f_color_gradient_from_moments_host: host-only twin of everything after the moments (the same inline code): m[13],
 * Q, nrm[3], the point's own intensity, min_neighbors -> out[4], one row of `field`.
 *
 * d3f_icp_rigid_color: d3f_icp_rigid_plane with `field` [Ns,4] f32 (16-byte aligned) and lambda_geometric in [0, 1].
 * Setup, search, n_k, sum d2, fitness, rmse, the stopping rule, trace, flags, block prefix and every reduction order
 * are d3f_icp_rigid_plane's.  Per accepted row a, c, J, r are point-to-plane's; J and r are multiplied by
 * sg = sqrt(lambda_geometric) before any product is formed.  A colour row is added when field[y] of the matched FIXED
 * point is finite in all four entries (d, I_y) and field[x].w = I_x of the moving point is finite:
 *   J_C = sc [a x d, d],  r_C = sc ((I_y - I_x) + (a - c) . d),  sc = sqrt(1 - lambda_geometric),
 * into the same 21 + 6 sums, after the geometric row.
 *   sums[31] = { the 29 of d3f_icp_rigid_plane over both kinds of rows, n_color,
 *                sum ((I_y - I_x) + (a - c) . d)^2 (unweighted) }.
 * Fit: d3f_icp_rigid_plane's on the first 29 (a singular system ends the pair with D3F_ICP_ST_SINGULAR).  Beside the
 * outputs of d3f_icp_rigid_plane: n_color [P] int32 and color_rmse [P] f64 = sqrt(sums[30] / n_color) (0 without colour
 * rows) of the RETURNED pose (0 for a pair the setup stopped), so that a caller sees whether colour took part.
 * lambda_geometric = 1: sg is exactly 1 and the colour rows add +-0 to accumulators that start at +0 -- T, count, rmse,
 * iterations, status and trace are d3f_icp_rigid_plane's bit for bit.  A field that is NaN everywhere gives
 * point-to-plane scaled by sg: n_color = 0.  Workspace: d3f_icp_rigid_color_ws_bytes(P, rows).  Launches, determinism
 * and batch independence as for d3f_icp_rigid.
 * ---------------------------------------------------------------------------------------------- */
int d3f_color_gradients(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                        float grid_radius, float radius, int min_neighbors, const float* normals,
                        const float* intensity, float* field, int32_t* count, int64_t* moments, int32_t* status,
                        void* stream);
int d3f_color_gradient_from_moments_host(const int64_t* m_host, double Q, const float* nrm_host, float intensity,
                                         int min_neighbors, float* out_host);
size_t d3f_icp_rigid_color_ws_bytes(int P, int64_t rows);
int d3f_icp_rigid_color(const void* grid_ws, const float* points, const float* normals, const float* field, int Ns,
                        const int32_t* cloud_start, int B, float grid_radius, float max_distance, const int32_t* pairs,
                        const int64_t* row_start, int P, int64_t rows, const double* T_init, double lambda_geometric,
                        int max_iters, double rel_fitness, double rel_rmse, double* T, int32_t* count, double* rmse,
                        int32_t* iterations, int32_t* status, int32_t* n_color, double* color_rmse, double* trace,
                        void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FPFH descriptors (Rusu, Blodow, Beetz 2009) of every point of the stacked clouds of a cell list: the training-free
 * descriptor of the registration chain.  Replaces Open3D's compute_fpfh_feature, which the reference's users run on the
 * CPU.  csrc/fpfh.hpp states the rule beside the code; in short:
 *   neighbours of point i: the points j != i of the SAME cloud with d2 < radius * radius (f32 without FMA, strict: the
 *        acceptance of d3f_estimate_normals), a normal that is not (0, 0, 0), and a non-zero f64 distance; a point whose
 *        own normal is (0, 0, 0) has no descriptor and is nobody's neighbour; n_i = the number of neighbours;
 *   pair features in f64 with + - * / sqrt only, Open3D's role swap decided by |a1| < |a2|, the angle's bin decided by
 *        the signs of ten 2x2 determinants against constant (cos, sin) pairs -- no acos, no atan2;
 *   SPFH: c_i[33] int32 counts (theta, f2, f3; 11 bins each);
 *   FPFH: W_j = (int64) rint((2^32 min(radius^2 / d2, 2^12)) / n_j), S_i[b] = sum_j W_j c_j[b] in int64,
 *        desc_i[b] = f32((100 S_i[b]) / tot_h + (100 c_i[b]) / n_i), tot_h the sum of b's histogram of S_i.
 * Every sum over neighbours is an integer, so the result is bit-identical from run to run, for any row order, for a
 * cloud alone or stacked, and for any cell size.  The cap 2^12 on the weight (a neighbour closer than radius / 64) and
 * the omission of atan2 / acos are the two differences from Open3D.
 *
 * d3f_fpfh.  The cell list (grid_ws, grid_radius), points, Ns, cloud_start and B are those of d3f_estimate_normals;
 * radius <= grid_radius; `normals` [Ns,3] f32 in input row order; row_width 33 or 64 (columns 33.. are zeros: the width
 * d3f_mutual_nn reads); unit != 0 scales every row to unit L2 norm -- unit_i[b] = f32(desc_i[b] / sqrt(q)) in f64, q the
 * sum of the squares of the 33 f32 entries in the order b = 0..32 -- which d3f_mutual_nn needs: it ranks by the inner
 * product of unit rows.  Outputs in input row order: desc [Ns,row_width] f32, count [Ns] int32 (= n_i), optional (NULL
 * to skip) spfh [Ns,33] int32.  A point without a descriptor (n_i = 0: no usable normal, no neighbour, or outside the
 * addressable cell grid, which also sets D3F_ST_CELL_RANGE in *status) and the rows beyond cloud_start[B] get zeros and
 * count 0.  A point with more than 2^18 neighbours, beyond which the int64 sums could overflow, sets
 * D3F_ST_CAND_OVERFLOW in *status and gets zeros.  ws: d3f_fpfh_ws_bytes(Ns) bytes, 16-byte aligned (the SPFH table
 * between the two passes).  Two launches on `stream`, no host synchronisation, no allocation, no floating-point atomics.
 * d3f_fpfh_host: the same inline rule on the host over HOST arrays, brute force within each cloud (it knows no cell
 * grid, so no point is out of range).
 * ---------------------------------------------------------------------------------------------- */
size_t d3f_fpfh_ws_bytes(int Ns);
int d3f_fpfh(const void* grid_ws, const float* points, const float* normals, int Ns, const int32_t* cloud_start, int B,
             float grid_radius, float radius, int row_width, int unit, float* desc, int32_t* count, int32_t* spfh,
             int32_t* status, void* ws, size_t ws_bytes, void* stream);
/* measurement aid (profiles/fpfh_bench.py): d3f_fpfh with passes = 1 the SPFH launch alone, 2 the FPFH launch alone
 * over the table a previous call left in ws, 3 both (= d3f_fpfh) */
int d3f_fpfh_passes(const void* grid_ws, const float* points, const float* normals, int Ns, const int32_t* cloud_start,
                    int B, float grid_radius, float radius, int row_width, int unit, float* desc, int32_t* count,
                    int32_t* spfh, int32_t* status, void* ws, size_t ws_bytes, int passes, void* stream);
int d3f_fpfh_host(const float* points, const float* normals, int Ns, const int32_t* cloud_start, int B, float radius,
                  int row_width, int unit, float* desc, int32_t* count, int32_t* spfh);

/* ------------------------------------------------------------------------------------------------
 * ISS keypoints (Zhong 2009; Open3D's compute_iss_keypoints) of every point of the stacked clouds of a cell list, and
 * radius non-maximum suppression of ANY per-point score over the same list: the detector of the training-free chain and
 * the suppression a caller wraps around the learned detector's scores.  csrc/iss.hpp states the rule beside the code.
 *
 * d3f_iss_saliency.  The cell list (grid_ws, grid_radius), points, Ns, cloud_start, B and the neighbourhood at `radius`
 * (the salient radius) are those of d3f_estimate_normals bit for bit: the points j of the SAME cloud, i itself included,
 * with d2 < radius * radius (f32 without FMA, f32 product, strict), the same Q and the same ten int64 moments.
 *   C = (S - s s^T / n) / n / Q^2 in f64, formed as for the normals, and diagonalised by the same fixed number of cyclic
 *        Jacobi sweeps (csrc/plane.hpp) without eigenvectors; e1 >= e2 >= e3 its sorted diagonal;
 *   salient: n >= min_neighbors (>= 1), e1 > 0, e2 < gamma_21 e1, e3 < gamma_32 e2 (products in f64, no division;
 *        0 < gamma <= 1; Open3D's defaults are 0.975, 0.975 and 5);
 *   saliency = (float)e3 in squared length units when salient and that float is > 0, else 0.0f.
 * Outputs in input row order: saliency [Ns] f32, count [Ns] int32 (= n), optional (NULL to skip) moments [Ns,10] int64.
 * Rows beyond cloud_start[B] get zeros.  A point outside the addressable cell grid is in no cell list: zeros, and
 * D3F_ST_CELL_RANGE in *status.  The moments are integers, so the result does not depend on the order of the rows, on
 * the clouds stacked beside a cloud or on the cell size, and is bit-identical from run to run.
 * d3f_iss_saliency_from_moments_host: host-only twin of everything after the moments (the same inline code): m[10], Q,
 * the gammas and min_neighbors -> *out.
 *
 * d3f_radius_nms.  `score` [Ns] f32 in input row order, any values; `radius` (the non-maximum radius) <= grid_radius;
 * min_neighbors >= 1.  Row i is KEPT when
 *   score[i] > 0 (a NaN is not),
 *   no neighbour j (the acceptance above, at `radius`) has score[j] > score[i] -- strictly: equal scores both survive,
 *        so the result does not depend on the row order (Open3D's IsLocalMaxima); a NaN neighbour beats nobody,
 *   and the neighbourhood holds at least min_neighbors points, i included.
 * Outputs: keep [Ns] uint8 (0 / 1) and count [Ns] int32, the size of the neighbourhood.  A row whose score is not > 0,
 * a row outside the addressable grid (D3F_ST_CELL_RANGE) and the rows beyond cloud_start[B] are not searched: keep 0,
 * count 0.  Every other row is searched to the end, beaten or not, so count is its whole neighbourhood and both outputs
 * are a pure function of (points, score, radius, min_neighbors).  No arithmetic beyond the distance test.
 * d3f_radius_nms_host: the same rule on the host over HOST arrays, brute force within each cloud, one thread (it knows
 * no cell grid, so no point is out of range).
 *
 * d3f_iss_keypoints: d3f_iss_saliency at salient_radius, then d3f_radius_nms of that saliency at non_max_radius with the
 * same min_neighbors, on one stream over one cell list (grid_radius covers both radii).  Outputs those of the two.
 * Every entry: one launch per pass on `stream`, no workspace, no host synchronisation, no allocation, no LDS, no
 * floating-point atomics; capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
int d3f_iss_saliency(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                     float grid_radius, float radius, double gamma_21, double gamma_32, int min_neighbors,
                     float* saliency, int32_t* count, int64_t* moments, int32_t* status, void* stream);
int d3f_radius_nms(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                   float grid_radius, float radius, const float* score, int min_neighbors, uint8_t* keep,
                   int32_t* count, int32_t* status, void* stream);
int d3f_iss_keypoints(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                      float grid_radius, float salient_radius, float non_max_radius, double gamma_21, double gamma_32,
                      int min_neighbors, float* saliency, uint8_t* keep, int32_t* count_salient, int32_t* count_nms,
                      int32_t* status, void* stream);
int d3f_iss_saliency_from_moments_host(const int64_t* m_host, double Q, double gamma_21, double gamma_32,
                                       int min_neighbors, float* out_host);
int d3f_radius_nms_host(const float* points, const float* score, int Ns, const int32_t* cloud_start, int B,
                        float radius, int min_neighbors, uint8_t* keep, int32_t* count);

/* ------------------------------------------------------------------------------------------------
 * Raw moments of the accepted correspondences of cloud pairs under GIVEN poses -- what the 6x6 information matrix of a
 * pair is made of (the benchmark's gt.info, which registration recall is scored under, and the weight of an edge of a
 * pose graph; Open3D's get_information_matrix_from_point_clouds).  The clouds, the cell list (grid_ws, grid_radius),
 * cloud_start, pairs and row_start are those of d3f_icp_rigid: pair p = (pairs[2p] MOVING cloud a, pairs[2p+1] FIXED
 * cloud b) and T [P,12] f64 (row-major 3x4 per pair) maps points of a into b's frame.  For a gt.log key i_j the pair is
 * (j, i) with the gt.log matrix as it stands.
 *   1. ONE search under T with the arithmetic, acceptance (d2 < max_distance * max_distance, f32) and tie rule of
 *      d3f_nearest_pairs -- iteration 0 of d3f_icp_rigid.
 *   2. Over the accepted rows, in f64, with x the moving point's OWN f32 coordinates (not moved by T) and y the matched
 *      fixed point:
 *        moments[20] = { n, sum x (3), sum x x^T (xx, xy, xz, yy, yz, zz), sum y (3), sum y y^T (6), sum d2 }
 *      (the f32 d2 widened, as in ICP).  RAW moments, no pivots: a product of two f32 values is exact in f64 and nothing
 *      is subtracted afterwards.  With G = [I | -[p]x] the information matrix sum G^T G is
 *      [[n I, -[s]x], [[s]x, sum (|p|^2 I - p p^T)]], s = sum p: the benchmark's form takes p = x (the error
 *      D = inv(T_gt) T_est acts in the moving cloud's frame), Open3D's takes p = y and puts the rotation block first.
 * Outputs per pair: moments [P,20] f64; count [P] int32 (= n); status [P] int32 (D3F_ICP_ST_* bits).  A pair that names
 * a cloud outside [0, B), or whose rows reach beyond `rows`, gets D3F_ICP_ST_PAIR; a non-finite T D3F_ICP_ST_NONFINITE;
 * both give zero moments and count 0.  D3F_ICP_ST_CELL_RANGE as in d3f_icp_rigid.  A pair without an accepted row has
 * zero moments and status 0.
 * Deterministic and batch-independent by d3f_icp_rigid's orders: a workgroup serves D3F_ICP_BLOCK_ROWS consecutive rows
 * of ONE pair, lanes add in slice order, waves by the fixed butterfly and then in wave order, and a finishing launch
 * adds the pair's workgroups in the fit's order -- no floating-point atomics -- so a pair's moments are bit-identical
 * alone or inside any batch and from run to run.
 * `rows` >= row_start[P] sizes the launches and the workspace (d3f_pair_information_ws_bytes(P, rows)); P <= 65535,
 * max_distance <= grid_radius.  3 launches on `stream` whatever the data, no host synchronisation, no allocation
 * (graph-capturable).
 * ---------------------------------------------------------------------------------------------- */
#define D3F_INFO_MOMENTS 20
size_t d3f_pair_information_ws_bytes(int P, int64_t rows);
int d3f_pair_information(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                         float grid_radius, float max_distance, const int32_t* pairs, const int64_t* row_start, int P,
                         int64_t rows, const double* T, double* moments, int32_t* count, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multiway registration: robust pose-graph optimisation of the fragments of a scene -- the step the 3DMatch / Open3D
 * reconstruction pipeline ends with (Levenberg-Marquardt on SE(3) with the line process of Choi, Zhou, Koltun 2015 on
 * the uncertain edges, pruning, a second pass).  The reference has no counterpart.  csrc/posegraph.hpp holds the text
 * the kernel and the host twin both run.
 *
 * A batch of G graphs is stacked: node_start [G+1] / edge_start [G+1] int32 delimit the graphs inside poses [N,16] and
 * the edge arrays [E,...]; edges [E,2] int32 = (i, j), indices LOCAL to the graph, i != j; (j, i) with j > i and
 * duplicates are legal.  All matrices f64 row-major.
 *   node k:  pose P_k (4x4, rigid) maps fragment k into the frame of its component's reference node;
 *   edge e:  Z_e (4x4) maps fragment j into fragment i (gt.log's key i_j, what d3f_ransac_rigid returns, inv(P_i) P_j);
 *            L_e (6x6, symmetric) in the moving frame with the translation block first (the gt.info form, the frame
 *            D = inv(T_gt) T_est acts in); uncertain[e] != 0 puts the edge under the line process.
 *   inv() is the rigid inverse [R^T, -R^T t].
 *   D_e = inv(Z_e) inv(P_i) P_j;  r_e = [D_t ; log(D_R)] (rotation vector);  c_e = r_e^T L_e r_e -- to first order the
 *   sum of squared displacements of the pair's correspondences, so mu below is in squared metres times a count.
 *   energy = sum over certain active edges of c_e + sum over uncertain active edges of mu c_e / (mu + c_e);
 *   weight l_e = (mu / (mu + c_e))^2 (uncertain), 1 (certain);
 *   mu = preference_loop_closure * max_distance^2 * mean over the graph's ACTIVE edges of L_e[0,0] (the number of
 *   correspondences), taken anew for each pass.
 *   update P_k <- P_k Exp(d_k), Exp([v, w]) = [[R(w), v], [0, 1]].
 * An edge whose L_e holds a non-finite value or has L_e[0,0] <= 0 is inactive from the start and reported pruned.
 * Components are taken over the active edges (min-label propagation); the lowest-numbered node of every component is
 * FIXED and its returned pose is bit-equal to the given one; an isolated node is its own component.
 * One call makes two passes: optimise; mark pruned (and deactivate) every uncertain edge with l_e < prune_threshold
 * (0.25 is c_e > mu); recompute the components; optimise the remaining edges again.
 * A pass is Levenberg-Marquardt on the weighted normal equations, weights frozen within an iteration, Jacobians exact
 * (csrc/posegraph.hpp), damping relative to the diagonal:
 *   lambda = 1e-4 at the start of a pass; ITERATION (at most max_iters per pass):
 *     factor H + lambda diag(H) (dense f64 Cholesky, rows and columns of the fixed nodes identity); a pivot that is
 *       not > 0: lambda *= 10 and, beyond 1e8, the pass ends with D3F_PG_ST_INDEFINITE;
 *     d = -(H + lambda diag(H))^-1 g, trial poses, their energy E';
 *     E' < E: accepted, lambda = max(lambda / 10, 1e-12); the pass ends when max|d| <= step_tol or
 *       E - E' <= rel_cost * E;
 *     otherwise rejected: the pass ends when max|d| <= step_tol; lambda *= 10 and, beyond 1e8, the pass ends.
 *   A pass that used max_iters iterations without ending sets D3F_PG_ST_ITER_CAP.  The Python layer's defaults:
 *   preference_loop_closure 2, prune_threshold 0.25, max_iters 100, step_tol 1e-9, rel_cost 1e-9.
 * Outputs: out_poses [N,16]; weight [E] = l_e at the end of the last pass in which the edge was active (0 for an edge
 * inactive from the start); pruned [E] int32; component [N] int32 = the lowest node (local index) of the node's
 * component after pruning; iterations [G,2] per pass; cost [G,3] = energy at the start, after pass 1 (under pass 1's
 * mu), at the end (under pass 2's mu); status [G] = D3F_PG_ST_* bits.  A graph with a non-finite pose or measurement
 * (D3F_PG_ST_NONFINITE), or with an edge index outside the graph, i == j, or more nodes / edges than max_nodes /
 * max_edges (D3F_PG_ST_GRAPH) returns its poses as given, zero weights and iterations and every node its own component.
 * max_nodes / max_edges are host bounds on ONE graph's size; they size the workspace
 * (d3f_pose_graph_optimize_ws_bytes(G, max_nodes, max_edges): two dense [6 max_nodes]^2 matrices and 1 KB per edge,
 * per graph).  max_nodes <= D3F_PG_MAX_NODES = 128 (D3F_EINVAL beyond): the 6-row panel of the factorisation
 * (6 x 6 max_nodes f64) and the step vector live in LDS, 43 KB at the cap, and the matrices of a larger graph would
 * leave L2.  G <= 65535, max_edges <= 2^20, max_iters <= 1024.
 * One workgroup per graph carries both passes: ONE launch on `stream`, no host synchronisation, no allocation
 * (graph-capturable).  Every entry of H and g has one owner that adds the node's edges in ascending edge order and
 * every energy is summed in one fixed shape -- no floating-point atomics -- so a graph's result is bit-identical from
 * run to run, alone or inside any batch.
 * d3f_pose_graph_optimize_host: the host twin -- the same arguments as host pointers, the same text run by one
 * worker, no GPU call (`stream` is ignored).  It differs from the device only where sin / cos / atan2 / sqrt do.
 * d3f_pose_graph_edge_host: one edge: r [6], *cost = c_e, Ji / Jj [36] row-major (row = residual component,
 * column = component of d_i / d_j).
 * ---------------------------------------------------------------------------------------------- */
#define D3F_PG_MAX_NODES 128
#define D3F_PG_MAX_EDGES (1 << 20)
#define D3F_PG_MAX_GRAPHS 65535
#define D3F_PG_MAX_ITERS 1024
#define D3F_PG_ST_ITER_CAP 1    /* a pass used max_iters iterations without meeting a stopping rule */
#define D3F_PG_ST_NONFINITE 2   /* a pose or a measurement holds a non-finite value: poses returned as given */
#define D3F_PG_ST_GRAPH 4       /* an edge index out of range, i == j, or a graph beyond max_nodes / max_edges */
#define D3F_PG_ST_INDEFINITE 8  /* the normal equations stayed indefinite at the largest damping */
size_t d3f_pose_graph_optimize_ws_bytes(int G, int max_nodes, int max_edges);
int d3f_pose_graph_optimize(const int32_t* node_start, const int32_t* edge_start, int G, int N, int E, int max_nodes,
                            int max_edges, const double* poses, const int32_t* edges, const double* Z,
                            const double* info, const int32_t* uncertain, double max_distance,
                            double preference_loop_closure, double prune_threshold, int max_iters, double step_tol,
                            double rel_cost, double* out_poses, double* weight, int32_t* pruned, int32_t* component,
                            int32_t* iterations, double* cost, int32_t* status, void* ws, size_t ws_bytes,
                            void* stream);
int d3f_pose_graph_optimize_host(const int32_t* node_start, const int32_t* edge_start, int G, int N, int E,
                                 int max_nodes, int max_edges, const double* poses, const int32_t* edges,
                                 const double* Z, const double* info, const int32_t* uncertain, double max_distance,
                                 double preference_loop_closure, double prune_threshold, int max_iters,
                                 double step_tol, double rel_cost, double* out_poses, double* weight, int32_t* pruned,
                                 int32_t* component, int32_t* iterations, double* cost, int32_t* status, void* ws,
                                 size_t ws_bytes, void* stream);
int d3f_pose_graph_edge_host(const double* Pi_host, const double* Pj_host, const double* Z_host, const double* L_host,
                             double* r_host, double* cost_host, double* Ji_host, double* Jj_host);

/* ------------------------------------------------------------------------------------------------
 * TSDF fusion of depth frames into a batch of V dense volumes, and the extraction of their zero crossings as point
 * clouds (csrc/tsdf.hpp states the rule in full; the reference has no such step).  The bounds are csrc/tsdf.hip,
 * the integration csrc/tsdf_integrate.hip, the extraction csrc/tsdf_extract.hip.
 * Volume v: lattice dims[v] = (nx, ny, nz), ix fastest; origin[v][3], voxel[v], trunc[v]; its voxels are
 * [vol_start[v], vol_start[v+1]) of D / w (vol_start int64 [V+1] from 0 to total_voxels; every dim >= 1); it owns the
 * frames [frame_start[v], frame_start[v+1]) (an empty range leaves the volume at D = 0, w = 0).
 * Frames: depth [F, H, W] uint16 raw units (metres = raw / depth_scale) or f32 metres (depth_is_f32), intrinsics
 * [F, 4] = fx, fy, cx, cy, volume_to_camera / camera_to_volume [F, 12] row-major 3x4 f32.  A pixel is valid when
 * d > 0 and not d > depth_max.  All arithmetic f32 in the order of tsdf.hpp; device, host twin and the NumPy
 * restatement agree bit for bit.
 * d3f_tsdf_bounds: bounds [V, 6] = per volume the minimum (3) and maximum (3) of the back-projected valid pixels of
 *   its frames in the volume's frame; +inf / -inf where there is none.  Integer-ordered min / max atomics: exact.
 *   F <= 65535.
 * d3f_tsdf_integrate: D, w f32 [total_voxels], written once by the thread that owns the voxel for all frames: no
 *   atomics, nothing read back, bit-identical from run to run and for a volume alone or inside any batch.
 *   max_volume_voxels: a host bound on the voxels of one volume (the launch is blocks of the largest volume x V, the
 *   volume being the grid's second index: uniform, so its frames' matrices come through scalar loads); voxels of a
 *   volume beyond it are not written.
 * The rules of the eight entries d3f_tsdf[_sparse]_integrate[_host] and d3f_tsdf_raycast[_sparse][_host]:
 *   channels is 0, 1 or 3; anything else is D3F_EINVAL, before anything else is looked at.  channels = 0 is the
 *     colourless form: color, Cv / Cp and the ray-cast's color image are not looked at and may be null.  With 1 or 3
 *     ("Colour in TSDF volumes" below) integrate needs Cv / Cp, and color when F > 0; a ray-cast with R > 0 needs the
 *     color image, and Cv / Cp when something is stored (total_voxels > 0, bricks > 0).
 *   into != 0 continues the running mean from the stored D, w (and Cv / Cp when channels > 0), which every cell's
 *     thread reads first; into = 0 starts from zero.  The mean is sequential over frames, so the frames [0, k) and
 *     then, into the result, [k, F) give the volume of one call over [0, F) bit for bit (sparse: for fixed tables).  A
 *     volume that owns no frame in an into call keeps its values, and so do a brick's slots beyond dims.
 *   A twin's parameter list is its device form's: it takes host pointers, makes no GPU call and ignores stream, the
 *     dense integrate twin max_volume_voxels too.
 *   An empty model (total_voxels = 0, max_volume_voxels = 0, bricks = 0) is D3F_OK before D, w and the colour pointers
 *     are looked at; R = 0 is D3F_OK before the colour pointers are looked at.
 *   Dense and sparse, all of integrate is one kernel body and one host function in csrc/tsdf_integrate.hip, all of
 *   ray-cast one of each in csrc/tsdf_raycast.hip.
 * d3f_tsdf_extract: count per block of voxels, exclusive scan, emit at block offset + in-block rank: points
 *   [capacity, 3] in the order volume, lattice index of the lower voxel, axis; point_start int64 [V+1].  A point at
 *   or beyond `capacity` is not written and ORs D3F_TSDF_ST_OVERFLOW into *status (int32, zeroed by the caller);
 *   point_start is complete either way.  d3f_tsdf_extract_count runs the first two steps alone and writes
 *   point_start[V] (the number of points); a following d3f_tsdf_extract on the same volumes and workspace with
 *   counted = 1 skips them.  vol_start is taken to be the prefix of dims; where they disagree the result is
 *   unspecified, but nothing outside a volume's own voxel range is read.
 * The _host twins take host pointers and make no GPU call.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_TSDF_MAX_VOLUMES 65535
#define D3F_TSDF_ST_OVERFLOW 1
int d3f_tsdf_bounds(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start, int V,
                    const float* intrinsics, const float* camera_to_volume, float depth_scale, float depth_max,
                    float* bounds, void* stream);
int d3f_tsdf_bounds_host(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start, int V,
                         const float* intrinsics, const float* camera_to_volume, float depth_scale, float depth_max,
                         float* bounds, void* stream);
int d3f_tsdf_integrate(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H, int W,
                       const int32_t* frame_start, const int64_t* vol_start, int V, int64_t total_voxels,
                       int64_t max_volume_voxels, const float* intrinsics, const float* volume_to_camera,
                       const float* origin, const int32_t* dims, const float* voxel, const float* trunc,
                       float depth_scale, float depth_max, int into, float* D, float* w, float* Cv, void* stream);
int d3f_tsdf_integrate_host(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H, int W,
                            const int32_t* frame_start, const int64_t* vol_start, int V, int64_t total_voxels,
                            int64_t max_volume_voxels, const float* intrinsics, const float* volume_to_camera,
                            const float* origin, const int32_t* dims, const float* voxel, const float* trunc,
                            float depth_scale, float depth_max, int into, float* D, float* w, float* Cv, void* stream);
size_t d3f_tsdf_extract_ws_bytes(int64_t total_voxels);
int d3f_tsdf_extract_count(const float* D, const float* w, const int64_t* vol_start, const int32_t* dims, int V,
                           int64_t total_voxels, float min_weight, int64_t* point_start, void* ws, size_t ws_bytes,
                           void* stream);
int d3f_tsdf_extract(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                     const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                     int counted, int64_t capacity, float* points, int64_t* point_start, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream);
int d3f_tsdf_extract_host(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                          int64_t capacity, float* points, int64_t* point_start, int32_t* status);

/* ------------------------------------------------------------------------------------------------
 * Sparse TSDF volumes: the same batch of V volumes, frames and rule, but D and w are kept only for the bricks of
 * 8 x 8 x 8 voxels that a depth pixel can reach within trunc (csrc/tsdf_sparse.hpp states the rule in full, with the
 * argument that no voxel the dense volume can emit a point from is left out; the reference has no such step).
 * Volume v has a brick lattice of ceil(n / 8) bricks per axis, bx fastest: the lattice bricks of the batch are
 * [lattice_start[v], lattice_start[v+1]) of flags / brick_index (lattice_start int64 [V+1] from 0 to lattice_bricks,
 * the prefix of the volumes' brick lattices; lattice_bricks <= 2^31 - 1).  Its allocated bricks are the pool rows
 * [brick_start[v], brick_start[v+1]) (int64 [V+1] from 0 to `bricks`), in lattice order; brick_coord [bricks, 3] =
 * (bx, by, bz) of a row; brick_index [lattice_bricks] = the rank of a lattice brick among the allocated bricks of its
 * volume, or -1.  The pool D, w is f32 [bricks, 512]: voxel (ix, iy, iz) at slot (ix & 7) + 8 (iy & 7) + 64 (iz & 7)
 * of its brick's row; a slot beyond dims holds D = 0, w = 0.  The other arguments are those of the dense entry points.
 * d3f_tsdf_sparse_mark: flags int32 [lattice_bricks], zeroed here, then 1 for every brick in the box of a valid pixel
 *   (plain idempotent stores: the result is a set, no atomic decides anything).  F <= 65535.
 * d3f_tsdf_sparse_index: exclusive scan of the flags (as mark wrote them, 0 / 1) -> brick_index, brick_start
 *   (brick_start[V] = the number of allocated bricks, the one value a caller reads back) and brick_coord, which must
 *   hold lattice_bricks rows (the bound known before the read-back); the rows from brick_start[V] on are not written.
 * d3f_tsdf_sparse_integrate: one workgroup per pool row, written once by the threads that own its slots for all frames
 *   of the row's volume: no atomics, nothing read back; every slot is d3f_tsdf_integrate's voxel bit for bit.  color,
 *   channels and into follow the rules stated there; a slot beyond dims holds colour 0 beside D = 0, w = 0.
 * d3f_tsdf_sparse_extract: count per block of 256 slots, exclusive scan, emit, as d3f_tsdf_extract; the +1 neighbour
 *   across a brick face is found through brick_index, an absent brick being an invalid neighbour.  points
 *   [capacity, 3] in the order volume, brick in lattice order, slot, axis: d3f_tsdf_extract's rows bit for bit, as a
 *   set.  capacity, status, counted, d3f_tsdf_sparse_extract_count and point_start as for d3f_tsdf_extract; bricks >= 1.
 *   Indices read from brick_index / brick_coord / brick_start are bounded before use: tables that disagree with each
 *   other give an unspecified result, but nothing outside brick_index and the pool is read.
 * The _host twins take host pointers and make no GPU call.
 * ---------------------------------------------------------------------------------------------- */
int d3f_tsdf_sparse_mark(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start, int V,
                         const float* intrinsics, const float* camera_to_volume, const float* origin,
                         const int32_t* dims, const float* voxel, const float* trunc, const int64_t* lattice_start,
                         int64_t lattice_bricks, float depth_scale, float depth_max, int32_t* flags, void* stream);
int d3f_tsdf_sparse_mark_host(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start,
                              int V, const float* intrinsics, const float* camera_to_volume, const float* origin,
                              const int32_t* dims, const float* voxel, const float* trunc,
                              const int64_t* lattice_start, int64_t lattice_bricks, float depth_scale, float depth_max,
                              int32_t* flags);
size_t d3f_tsdf_sparse_index_ws_bytes(int64_t lattice_bricks);
int d3f_tsdf_sparse_index(const int32_t* flags, const int64_t* lattice_start, const int32_t* dims, int V,
                          int64_t lattice_bricks, int32_t* brick_index, int32_t* brick_coord, int64_t* brick_start,
                          void* ws, size_t ws_bytes, void* stream);
int d3f_tsdf_sparse_index_host(const int32_t* flags, const int64_t* lattice_start, const int32_t* dims, int V,
                               int64_t lattice_bricks, int32_t* brick_index, int32_t* brick_coord,
                               int64_t* brick_start);
int d3f_tsdf_sparse_integrate(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H,
                              int W, const int32_t* frame_start, int V, const float* intrinsics,
                              const float* volume_to_camera, const float* origin, const int32_t* dims,
                              const float* voxel, const float* trunc, const int64_t* brick_start,
                              const int32_t* brick_coord, int64_t bricks, float depth_scale, float depth_max,
                              int into, float* D, float* w, float* Cp, void* stream);
int d3f_tsdf_sparse_integrate_host(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H,
                                   int W, const int32_t* frame_start, int V, const float* intrinsics,
                                   const float* volume_to_camera, const float* origin, const int32_t* dims,
                                   const float* voxel, const float* trunc, const int64_t* brick_start,
                                   const int32_t* brick_coord, int64_t bricks, float depth_scale, float depth_max,
                                   int into, float* D, float* w, float* Cp, void* stream);
size_t d3f_tsdf_sparse_extract_ws_bytes(int64_t bricks);
int d3f_tsdf_sparse_extract_count(const float* D, const float* w, const int64_t* lattice_start,
                                  const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                                  const int32_t* dims, int V, int64_t lattice_bricks, int64_t bricks, float min_weight,
                                  int64_t* point_start, void* ws, size_t ws_bytes, void* stream);
int d3f_tsdf_sparse_extract(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                            const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                            const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                            float min_weight, int counted, int64_t capacity, float* points, int64_t* point_start,
                            int32_t* status, void* ws, size_t ws_bytes, void* stream);
int d3f_tsdf_sparse_extract_host(const float* D, const float* w, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                                 const float* origin, const int32_t* dims, const float* voxel, int V,
                                 int64_t lattice_bricks, int64_t bricks, float min_weight, int64_t capacity,
                                 float* points, int64_t* point_start, int32_t* status);

/* ------------------------------------------------------------------------------------------------
 * Triangle meshes with normals from the same batch of TSDF volumes: dual contouring of the lattice ("naive surface
 * nets"; csrc/tsdf_mesh.hpp states the rule in full, in the terms of csrc/tsdf.hpp; the reference has no such step).
 * The arguments D, w, vol_start, origin, dims, voxel, V, total_voxels and min_weight are those of d3f_tsdf_extract.
 * A cell (the cube above a voxel) whose 8 corners are valid and that has a crossing edge owns one vertex: the mean of
 * the points d3f_tsdf_extract emits for its crossing edges, with the normalised gradient of D over the cell as its
 * normal (towards positive D: free space).  A crossing lattice edge whose four cells are complete emits a quad as two
 * triangles, counter-clockwise seen from positive D.  All arithmetic f32 in the order of tsdf_mesh.hpp; device, host
 * twin and the NumPy restatement agree bit for bit.
 * d3f_tsdf_mesh: count per block of voxels (vertices and triangles in one pass, keeping one bit per voxel), exclusive
 *   scans, emit at block offset + in-block rank: vertices and normals f32 [vertex_capacity, 3] in the order volume, cell
 *   index; faces int32 [face_capacity, 3] in the order volume, lattice index of the edge's lower voxel, axis, a quad's
 *   two triangles consecutive, their entries vertex indices LOCAL to the volume (global row = entry +
 *   vertex_start[v]); vertex_start, face_start int64 [V+1].  A vertex at or beyond vertex_capacity is not written and
 *   ORs D3F_TSDF_ST_OVERFLOW into *status (int32, zeroed by the caller), a triangle at or beyond face_capacity is not
 *   written and ORs D3F_TSDF_ST_FACE_OVERFLOW; both starts are complete either way.  A volume with more than 2^31 - 1
 *   vertices sets D3F_TSDF_ST_OVERFLOW instead of writing a wrapped index.  d3f_tsdf_mesh_count runs the count and the
 *   scans alone and writes vertex_start[V] and face_start[V] (the totals); a following d3f_tsdf_mesh on the same
 *   volumes and workspace with counted = 1 skips them.  Nothing outside a volume's own voxel range is read.
 * d3f_tsdf_mesh_host takes host pointers and makes no GPU call.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_TSDF_ST_FACE_OVERFLOW 2
size_t d3f_tsdf_mesh_ws_bytes(int64_t total_voxels);
int d3f_tsdf_mesh_count(const float* D, const float* w, const int64_t* vol_start, const int32_t* dims, int V,
                        int64_t total_voxels, float min_weight, int64_t* vertex_start, int64_t* face_start, void* ws,
                        size_t ws_bytes, void* stream);
int d3f_tsdf_mesh(const float* D, const float* w, const int64_t* vol_start, const float* origin, const int32_t* dims,
                  const float* voxel, int V, int64_t total_voxels, float min_weight, int counted,
                  int64_t vertex_capacity, int64_t face_capacity, float* vertices, float* normals, int32_t* faces,
                  int64_t* vertex_start, int64_t* face_start, int32_t* status, void* ws, size_t ws_bytes,
                  void* stream);
int d3f_tsdf_mesh_host(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                       const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                       int64_t vertex_capacity, int64_t face_capacity, float* vertices, float* normals, int32_t* faces,
                       int64_t* vertex_start, int64_t* face_start, int32_t* status);

/* ------------------------------------------------------------------------------------------------
 * Triangle meshes with normals straight from a sparse pool (csrc/tsdf_mesh_sparse.hpp states the rule in full, in the
 * terms of csrc/tsdf_mesh.hpp and csrc/tsdf_sparse.hpp; the reference has no such step).  The rule is d3f_tsdf_mesh's
 * with one thing replaced: a voxel's D and w come from its brick's pool row, and a voxel of an absent brick, a slot
 * beyond dims and a voxel outside the lattice are never valid.  The result is d3f_tsdf_mesh of the densified pool
 * (min_weight > 0): the same vertices, normals and faces bit for bit, in another order.  No dense array is built.
 * The arguments D, w [bricks, 512], lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V,
 * lattice_bricks, bricks and min_weight are those of d3f_tsdf_sparse_extract; the outputs, the capacities, status and
 * counted are those of d3f_tsdf_mesh.
 * d3f_tsdf_sparse_mesh: one workgroup per pool row, which looks up the up to 27 bricks around its own once and stages
 *   the 10 x 10 x 10 voxels around the brick in LDS; count per row (keeping one bit per slot), exclusive scans, emit at
 *   row offset + rank inside the row: vertices and normals f32 [vertex_capacity, 3] in the order volume, pool row
 *   (brick in lattice order), slot of the cell's lowest voxel; faces int32 [face_capacity, 3] in the order volume, pool
 *   row and slot of the edge's lower voxel, axis, a quad's two triangles consecutive, their entries vertex indices
 *   LOCAL to the volume; vertex_start, face_start int64 [V+1], a volume without bricks owning an empty range.  A
 *   vertex at or beyond vertex_capacity is not written and ORs D3F_TSDF_ST_OVERFLOW into *status (int32, zeroed by the
 *   caller), a triangle at or beyond face_capacity is not written and ORs D3F_TSDF_ST_FACE_OVERFLOW; both starts are
 *   complete either way.  A volume with more than 2^31 - 1 vertices sets D3F_TSDF_ST_OVERFLOW instead of writing a
 *   wrapped index.  d3f_tsdf_sparse_mesh_count runs the count and the scans alone and writes both starts in full; a
 *   following d3f_tsdf_sparse_mesh on the same pool and workspace with counted = 1 skips them.  bricks >= 1.  Indices
 *   read from the tables are bounded before use: tables that disagree with each other give an unspecified result,
 *   but nothing outside brick_index, the tables and the pool is read.
 * d3f_tsdf_sparse_mesh_host takes host pointers, makes no GPU call and accepts bricks = 0.
 * ---------------------------------------------------------------------------------------------- */
size_t d3f_tsdf_sparse_mesh_ws_bytes(int64_t bricks);
int d3f_tsdf_sparse_mesh_count(const float* D, const float* w, const int64_t* lattice_start,
                               const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                               const int32_t* dims, int V, int64_t lattice_bricks, int64_t bricks, float min_weight,
                               int64_t* vertex_start, int64_t* face_start, void* ws, size_t ws_bytes, void* stream);
int d3f_tsdf_sparse_mesh(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                         const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                         const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                         float min_weight, int counted, int64_t vertex_capacity, int64_t face_capacity, float* vertices,
                         float* normals, int32_t* faces, int64_t* vertex_start, int64_t* face_start, int32_t* status,
                         void* ws, size_t ws_bytes, void* stream);
int d3f_tsdf_sparse_mesh_host(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                              const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                              const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                              float min_weight, int64_t vertex_capacity, int64_t face_capacity, float* vertices,
                              float* normals, int32_t* faces, int64_t* vertex_start, int64_t* face_start,
                              int32_t* status);

/* ------------------------------------------------------------------------------------------------
 * Ray-casting dense TSDF volumes: a volume plus a camera pose gives a depth image and, when asked, a normal image
 * (csrc/tsdf_raycast.hpp states the rule in full; the reference has no such step).  The batch of V volumes is that of
 * d3f_tsdf_integrate (D, w, vol_start, origin, dims, voxel).  View r looks at volume view_volume[r] (int32 [R], any
 * order, a volume any number of times; a value outside [0, V) gives an image of zeros) through intrinsics[r] = fx, fy,
 * cx, cy and camera_to_volume[r] [12] row-major 3x4 f32; step is f32 [V], the sample spacing of a volume's views along
 * the camera z-depth.  Every ray samples the trilinear D at z_k = depth_min + step k <= depth_max, a sample being valid
 * when all 8 corners of its cell have w >= min_weight; a valid positive sample followed by a valid non-positive one is
 * a hit at the interpolated zero, a valid negative sample not preceded by a valid positive one ends the ray without
 * one.  depth f32 [R, H, W] in metres, 0 without a hit; normals (may be null) f32 [R, H, W, 3] in the camera frame,
 * towards positive D, zeros where there is no hit or a gradient sample is invalid; Cv, channels and the color image
 * [R, H, W, channels] by the rules stated with d3f_tsdf_integrate and "Colour in TSDF volumes" below.  clip != 0 cuts
 * every ray's sample range to the lattice's box (widened: the result is the same bit for bit; clip = 0 is the switch
 * that proves it).  A step that is not > 0 or gives more than D3F_RAYCAST_MAX_SAMPLES samples casts nothing.
 * 0 <= R <= 65535, H W <= 2^30, 0 <= depth_min <= depth_max.  One thread per ray, a wave per 8 x 8 pixels, all views in
 * one launch; no atomics, nothing read back, a view's image bit-identical alone, in any batch and from run to run, and
 * to the host twin.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_RAYCAST_MAX_SAMPLES 65536
int d3f_tsdf_raycast(const float* D, const float* w, const float* Cv, int channels, const int64_t* vol_start,
                     const float* origin, const int32_t* dims, const float* voxel, int V, int64_t total_voxels,
                     const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                     const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                     float min_weight, int clip, float* depth, float* normals, float* color, void* stream);
int d3f_tsdf_raycast_host(const float* D, const float* w, const float* Cv, int channels, const int64_t* vol_start,
                          const float* origin, const int32_t* dims, const float* voxel, int V, int64_t total_voxels,
                          const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                          const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                          float min_weight, int clip, float* depth, float* normals, float* color, void* stream);
/* d3f_tsdf_raycast_sparse: the same render of V SPARSE volumes (the tables and the pool of the sparse section above;
 *   csrc/tsdf_raycast_sparse.hpp states the rule): cast_ray unchanged, a corner voxel's D and w read from its brick's
 *   pool row, D = 0, w = 0 where the brick is absent -- by definition d3f_tsdf_raycast of the densified pool, bit for
 *   bit, depth and normals.  D, w f32 [bricks, 512] (may be null when bricks == 0: every image is then 0 unless
 *   min_weight <= 0).  skip != 0 steps over the samples that stay inside an absent brick (only when min_weight > 0; the
 *   result is the same bit for bit, skip = 0 is the switch that proves it).  Every index read from the tables is
 *   bounded before use: tables that do not fit give an unspecified image, and nothing outside brick_index
 *   [lattice_bricks] and the pool is read.  The other arguments, limits and guarantees are d3f_tsdf_raycast's. */
int d3f_tsdf_raycast_sparse(const float* D, const float* w, const float* Cp, int channels,
                            const int64_t* lattice_start, const int64_t* brick_start, const int32_t* brick_index,
                            const float* origin, const int32_t* dims, const float* voxel, int V,
                            int64_t lattice_bricks, int64_t bricks, const int32_t* view_volume, int R, int H, int W,
                            const float* intrinsics, const float* camera_to_volume, const float* step,
                            float depth_min, float depth_max, float min_weight, int clip, int skip, float* depth,
                            float* normals, float* color, void* stream);
int d3f_tsdf_raycast_sparse_host(const float* D, const float* w, const float* Cp, int channels,
                                 const int64_t* lattice_start, const int64_t* brick_start,
                                 const int32_t* brick_index, const float* origin, const int32_t* dims,
                                 const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                                 const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                                 const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                                 float min_weight, int clip, int skip, float* depth, float* normals, float* color,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Colour in TSDF volumes (csrc/tsdf_color.hpp states the rule in full, in the terms of csrc/tsdf.hpp,
 * csrc/tsdf_sparse.hpp and csrc/tsdf_raycast.hpp; the reference has no such step).  A colour volume Cv is f32
 * [total_voxels, channels], channel last, beside D and w; a sparse pool Cp is f32 [bricks, 512, channels]; channels is
 * 1 (intensity) or 3 (R, G, B) -- in the integrate and ray-cast entries above also 0, for no colour at all -- and
 * anything else is D3F_EINVAL.  Colour frames are f32 [F, H, W, channels], registered to the depth pixel by pixel.
 * Integrate: there is one weight: on exactly the frames that update D and w, with the w from before the increment,
 * c = (c w + c_pixel) / (w + 1) per channel, c_pixel read bilinearly over the 2 x 2 pixels around the voxel's
 * projection (indices clamped into the image); D and w are the channels = 0 call's bit for bit.
 * Ray-cast: depth and normals are the channels = 0 call's bit for bit; color f32 [R, H, W, channels] holds, at a hit,
 * color_at of the hit point -- the trilinear mean of the cell's corners with w >= min_weight, renormalised over those
 * corners -- and NaN in every channel without a hit (NaN, not 0: the render goes into the intensity pyramid as it is
 * and the RGB-D tracker's finiteness test drops those pixels).
 * ---------------------------------------------------------------------------------------------- */
/* d3f_tsdf_sample_color / d3f_tsdf_sample_color_sparse: color_at at N arbitrary points, one thread per point -- what
 * colours the clouds of d3f_tsdf_extract / d3f_tsdf_sparse_extract and the vertices of d3f_tsdf_mesh /
 * d3f_tsdf_sparse_mesh, whose kernels and output orders they leave alone.  points f32 [N, 3] in the frame of the
 * point's volume; point_start int64 [V + 1] as those calls return it (point i belongs to the last volume v with
 * point_start[v] <= i; a point no volume owns gets NaN).  out f32 [N, channels]: NaN in every channel where the point
 * lies outside the lattice (a NaN coordinate does) or its cell has no corner with w >= min_weight. */
int d3f_tsdf_sample_color(const float* Cv, const float* w, int channels, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels, const float* points,
                          const int64_t* point_start, int64_t N, float min_weight, float* out, void* stream);
int d3f_tsdf_sample_color_host(const float* Cv, const float* w, int channels, const int64_t* vol_start,
                               const float* origin, const int32_t* dims, const float* voxel, int V,
                               int64_t total_voxels, const float* points, const int64_t* point_start, int64_t N,
                               float min_weight, float* out, void* stream);
int d3f_tsdf_sample_color_sparse(const float* Cp, const float* w, int channels, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                 const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks,
                                 int64_t bricks, const float* points, const int64_t* point_start, int64_t N,
                                 float min_weight, float* out, void* stream);
int d3f_tsdf_sample_color_sparse_host(const float* Cp, const float* w, int channels, const int64_t* lattice_start,
                                      const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                      const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks,
                                      int64_t bricks, const float* points, const int64_t* point_start, int64_t N,
                                      float min_weight, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth odometry: the camera poses of a depth sequence by frame-to-frame projective point-to-plane ICP over a depth
 * pyramid (KinectFusion's tracker; csrc/odometry.hpp states the rule in full, in the terms of csrc/tsdf.hpp and
 * csrc/plane.hpp; the reference has no such step).  Frames as for d3f_tsdf_integrate: depth [F, H, W] uint16 raw units
 * or f32 metres, intrinsics [F, 4]; a pixel is valid when d > 0 and not d > depth_max.
 * The packed pyramid is f32 [F, d3f_depth_pyramid_pixels(H, W, levels)]: the levels of a frame one after another,
 * level l being (H >> l) x (W >> l) pixels in raster order (depth in metres, 0 where invalid; a 2x2 block of the finer
 * level averaged over its valid pixels, 0 when they span more than depth_diff).  level_intrinsics is f32
 * [F, levels, 4].  1 <= levels <= D3F_ODO_MAX_LEVELS and every level has at least one pixel; H W <= 2^30.
 * Pair p = pairs[2p], pairs[2p+1] = (moving frame a, fixed frame b); T [12] row-major 3x4 f64 maps a's camera frame
 * into b's (d3f_icp_rigid's convention).  An association at level l under T (rounded to f32) projects every valid
 * pixel of a into b, takes b's pixel there with the normal computed from b's depth, and accepts it within
 * max_distance; the accepted pixels give the D3F_ODO_SUMS = 29 sums of the point-to-plane normal equations
 * { n, the 21 upper entries of sum J J^T row by row, sum J r (6), sum d2 }, J = [a x n, n] (rotation first, in frame
 * b), in f64.  depth_diff is the pyramid's (the normals use it again).
 * d3f_depth_pyramid: one launch per level, one thread per output pixel, and a launch for the intrinsics.  Device,
 *   host twin and the NumPy restatement agree bit for bit.
 * d3f_depth_odometry_step: ONE association at `level` under T [P, 12]: sums [P, 29] and, when index is given, int32
 *   [P, (H >> level) (W >> level)] = per moving pixel the raster index of the accepted fixed pixel or -1.  A pair that
 *   names a frame outside [0, F) or whose T is not finite gives zero sums and -1 everywhere.
 * d3f_depth_odometry: from T_init [P, 12], iterations_host[l] (a HOST array of `levels` counts, each in
 *   0..D3F_ODO_MAX_ITERS) iterations of associate + fit (plane_step of csrc/plane.hpp, pivot 0) at level l, coarsest
 *   level first; an iteration with fewer than 6 accepted pixels or a singular system leaves T unchanged.  One more
 *   association at level 0 under the final T gives count [P] int32, rmse [P] f64 = sqrt(sum d2 / count) and, when
 *   information is given, [P, 36] f64 = sum J J^T as a full 6x6.  T [P, 16] f64 (4x4).  status [P] int32:
 *   D3F_ODO_ST_FEW (the final association has fewer than 6 accepted pixels), D3F_ODO_ST_SINGULAR (the last fit at
 *   level 0 was singular), D3F_ODO_ST_PAIR (a frame outside [0, F)), D3F_ODO_ST_NONFINITE (a non-finite T_init); each
 *   of them leaves T = T_init and gives count 0, rmse 0 and a zero information matrix.  The launch sequence depends on
 *   levels and iterations_host alone: no host synchronisation, nothing read back, capturable into a graph.  P <= 65535.
 * Deterministic and batch-independent: a workgroup serves D3F_ODO_CHUNK consecutive raster pixels of ONE pair's moving
 *   image, sums them in a fixed order (lane, wave butterfly, waves in order), and one wave adds the pair's chunks in
 *   ascending order; no floating-point atomic.  A pair's result is bit-identical alone, in any batch, from run to run.
 * ws: d3f_depth_odometry_ws_bytes(P, H, W) bytes, for both device entry points.
 * The _host twins take host pointers, sum in raster order and make no GPU call.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_ODO_MAX_LEVELS 8
#define D3F_ODO_MAX_ITERS 1024
#define D3F_ODO_CHUNK 1024
#define D3F_ODO_SUMS 29
#define D3F_ODO_ST_FEW 1        /* = D3F_ICP_ST_FEW */
#define D3F_ODO_ST_PAIR 4       /* = D3F_ICP_ST_PAIR */
#define D3F_ODO_ST_NONFINITE 8  /* = D3F_ICP_ST_NONFINITE */
#define D3F_ODO_ST_SINGULAR 16  /* = D3F_ICP_ST_SINGULAR */
int64_t d3f_depth_pyramid_pixels(int H, int W, int levels);   /* pixels of one frame's pyramid; 0 for a bad shape */
int d3f_depth_pyramid(const void* depth, int depth_is_f32, int F, int H, int W, const float* intrinsics, int levels,
                      float depth_scale, float depth_max, float depth_diff, float* pyramid, float* level_intrinsics,
                      void* stream);
int d3f_depth_pyramid_host(const void* depth, int depth_is_f32, int F, int H, int W, const float* intrinsics,
                           int levels, float depth_scale, float depth_max, float depth_diff, float* pyramid,
                           float* level_intrinsics);
size_t d3f_depth_odometry_ws_bytes(int P, int H, int W);
int d3f_depth_odometry_step(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                            const int32_t* pairs, int P, const double* T, int level, float max_distance,
                            float depth_diff, double* sums, int32_t* index, void* ws, size_t ws_bytes, void* stream);
int d3f_depth_odometry_step_host(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                                 const int32_t* pairs, int P, const double* T, int level, float max_distance,
                                 float depth_diff, double* sums, int32_t* index);
int d3f_depth_odometry(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                       const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                       float max_distance, float depth_diff, double* T, int32_t* count, double* rmse, int32_t* status,
                       double* information, void* ws, size_t ws_bytes, void* stream);
int d3f_depth_odometry_host(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                            const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                            float max_distance, float depth_diff, double* T, int32_t* count, double* rmse,
                            int32_t* status, double* information);

/* ------------------------------------------------------------------------------------------------
 * RGB-D odometry: the depth odometry above with a photometric term, so that a view of a single plane, which leaves
 * the depth-only system singular, is tracked by its texture (the hybrid objective of Park, Zhou, Koltun 2017 after
 * Steinbruecker et al. 2011; it stands in for Open3D's compute_rgbd_odometry, which the reference's fragment maker
 * calls; csrc/rgbd_odometry.hpp states the rule in full, on top of csrc/odometry.hpp).
 * The intensity pyramid is a second packed f32 array [F, d3f_depth_pyramid_pixels(H, W, levels)] with the depth
 * pyramid's level table.  Level 0 from `color`: D3F_RGBD_COLOR_RGB8 uint8 [F, H, W, 3],
 * I = ((0.299 R + 0.587 G) + 0.114 B) / 255 in f32; D3F_RGBD_COLOR_GREY8 uint8 [F, H, W], I = v / 255;
 * D3F_RGBD_COLOR_F32 f32 [F, H, W] as it is.  A coarser pixel is the f32 sum of its 2x2 block in raster order divided
 * by 4.  There is no validity: a non-finite value propagates upwards and is excluded where it is read.
 * An association is d3f_depth_odometry_step's: the same accepted pixels and index.  An accepted pixel whose unrounded
 * projection has its 2x2 bilinear footprint and the central differences at it inside the fixed image, with every
 * intensity read finite, adds a second row J_I = [a x q, q], r_I = I_b(projection) - I_a(pixel), q the derivative of
 * the sampled intensity with respect to the point, both scaled by photo_weight (>= 0, finite; intensity in [0, 1]
 * against metres).  D3F_RGBD_SUMS = 31 sums per pair: the 29 above, with sum J J^T and sum J r over both kinds of rows
 * and n, sum d2 geometric as before, then n_photo and sum r_I^2 (unweighted).  photo_weight = 0 skips the term:
 * n_photo = 0 and everything else equals the depth odometry's bit for bit.
 * d3f_rgbd_pyramid: the intensity pyramid alone (the depth pyramid and the intrinsics are d3f_depth_pyramid's); one
 *   launch per level, one thread per output pixel.  Device, host twin and the NumPy restatement agree bit for bit.
 * d3f_rgbd_odometry_step: ONE association at `level` under T [P, 12]: sums [P, 31] and the index as above.
 * d3f_rgbd_odometry: d3f_depth_odometry's schedule, outputs and statuses (D3F_ODO_ST_FEW by the geometric count,
 *   D3F_ODO_ST_SINGULAR by the combined system), information = the combined sum J J^T, and n_photo [P] int32 of the
 *   final association (0 with a status).  Same determinism and batch independence; no host synchronisation.
 * ws: d3f_rgbd_odometry_ws_bytes(P, H, W) bytes, for both device entry points.
 * The _host twins take host pointers, sum in raster order and make no GPU call.
 * ---------------------------------------------------------------------------------------------- */
#define D3F_RGBD_SUMS 31
#define D3F_RGBD_COLOR_RGB8 0
#define D3F_RGBD_COLOR_GREY8 1
#define D3F_RGBD_COLOR_F32 2
int d3f_rgbd_pyramid(const void* color, int color_kind, int F, int H, int W, int levels, float* intensity,
                     void* stream);
int d3f_rgbd_pyramid_host(const void* color, int color_kind, int F, int H, int W, int levels, float* intensity);
size_t d3f_rgbd_odometry_ws_bytes(int P, int H, int W);
int d3f_rgbd_odometry_step(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H,
                           int W, int levels, const int32_t* pairs, int P, const double* T, int level,
                           float max_distance, float depth_diff, float photo_weight, double* sums, int32_t* index,
                           void* ws, size_t ws_bytes, void* stream);
int d3f_rgbd_odometry_step_host(const float* pyramid, const float* intensity, const float* level_intrinsics, int F,
                                int H, int W, int levels, const int32_t* pairs, int P, const double* T, int level,
                                float max_distance, float depth_diff, float photo_weight, double* sums,
                                int32_t* index);
int d3f_rgbd_odometry(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H, int W,
                      int levels, const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                      float max_distance, float depth_diff, float photo_weight, double* T, int32_t* count, double* rmse,
                      int32_t* status, int32_t* n_photo, double* information, void* ws, size_t ws_bytes, void* stream);
int d3f_rgbd_odometry_host(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H,
                           int W, int levels, const int32_t* pairs, int P, const double* T_init,
                           const int32_t* iterations_host, float max_distance, float depth_diff, float photo_weight,
                           double* T, int32_t* count, double* rmse, int32_t* status, int32_t* n_photo,
                           double* information);

/* ------------------------------------------------------------------------------------------------
 * KPConv with the non-default influence / aggregation modes -- models/blocks.py:327-352 (KP_influence 'constant' /
 * 'gaussian', aggregation_mode 'closest'; the D3Feat configuration uses 'linear' / 'sum', config.py:39,41, which the
 * fused entry points above implement).  mode = influence (0 linear, 1 constant, 2 gaussian) | 4 for 'closest'.
 * The caller contracts with the kernel weights by plain GEMMs:
 *   forward : wf = aggregate_modes(...);  out = (wf @ W.view(K*Cin, Cout)) / nn
 *   backward: gwf = (grad_out / nn) @ W^T;  grad_W = wf^T (grad_out / nn);  grad_x = grad_input_modes(gwf)
 * wf_out [Nq, K*Cin], nn_out [Nq], gwf [Nq, K*Cin], grad_x [Ns, Cin] (overwritten).  Cin <= 512, K <= 16.
 * ---------------------------------------------------------------------------------------------- */
int d3f_kpconv_aggregate_modes(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                               const float* x, int Cin, const float* kernel_points, int K, float extent, int mode,
                               float* wf_out, float* nn_out, void* stream);
int d3f_kpconv_grad_input_modes(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* idx, int H,
                                int Cin, const float* kernel_points, int K, float extent, int mode, const float* gwf,
                                float* grad_x, void* stream);
/* For the deterministic mode: replaces the float-atomic scatter of d3f_kpconv_grad_input_modes (and, with mode 0, of the
 * general path of d3f_kpconv_backward) by a gather over the table's transpose -- CSR (rev_ptr [Ns+1] + rev_ent, rev_rel
 * NULL) or the exact form (rev_rel [Ns, rev_width, 4]) of d3f_kpconv_grad_input_gather.  One wave per support row adds
 * the row's edges in the transpose's order; grad_x [Ns, Cin] is overwritten.  Any Cin <= 512, K <= 16, every mode. */
int d3f_kpconv_grad_input_modes_gather(const float* q_pts, int Nq, const float* s_pts, int Ns, const int32_t* rev_ptr,
                                       const int32_t* rev_ent, const float* rev_rel, int rev_width, int Cin,
                                       const float* kernel_points, int K, float extent, int mode, const float* gwf,
                                       float* grad_x, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer step with the reference's non-finite-gradient guard -- replaces trainer.py:104-111 (per-parameter
 * torch.isfinite(...).all() host checks, then optimizer.step()) + torch.optim.SGD(momentum, weight_decay) as
 * configured in training_3DMatch.py:62-76, on flat fp32 buffers of n elements (16-byte aligned):
 *   if every grad[i] is finite:  buf = momentum*buf + (grad + weight_decay*params);  params -= lr*buf
 *   else: nothing is modified and state[1] (skipped-step counter) is incremented.
 * state: int32[4] on the device; state[0] is scratch, state[2] / state[3] collect the flags / the number of steps
 * skipped because pair_status (optional, device int32[1]: the status word of the pair the gradient came from --
 * capacity or candidate overflow of its pyramid) was set: such a gradient is treated like a non-finite one.
 * hyper_device: NULL, or float[4] on the device = {lr, momentum, weight_decay, grad_scale}, read when the kernel
 * executes in place of the scalar arguments (grad_scale multiplies the gradient first: 1/world_size turns an
 * all-reduced SUM into the mean without a pass of its own) -- the learning-rate schedule (ExponentialLR, training_3DMatch.py:78-81 stepped at
 * trainer.py:59-60) then changes the step size of an already captured hipGraph.
 * ---------------------------------------------------------------------------------------------- */
int d3f_sgd_guarded_step(const float* grad, float* params, float* momentum_buf, size_t n, float lr, float momentum,
                         float weight_decay, const float* hyper_device, int32_t* state, const int32_t* pair_status,
                         void* stream);
/* The same step on the SUM of n_grads (1..4) gradient buffers -- `grads` is a host array of device pointers, one buffer
 * per pair in flight on this GPU (train.PairLanes: several network steps run concurrently on streams of their own and
 * meet at one optimizer step, the update a data-parallel step over as many ranks makes).  Every buffer is tested for
 * non-finite values on its own; the sum is formed inside the update kernel (no pass of its own). */
int d3f_sgd_guarded_step_lanes(const float* const* grads, int n_grads, float* params, float* momentum_buf, size_t n,
                               float lr, float momentum, float weight_decay, const float* hyper_device, int32_t* state,
                               const int32_t* pair_status, void* stream);
/* Guarded Adam -- replaces torch.optim.Adam(lr, betas=(0.9, 0.999), weight_decay) as training_3DMatch.py:69-75
 * configures it for optimizer 'ADAM' (amsgrad off, L2 weight decay), with the same guard, state and pair_status as
 * the SGD step, on the SUM of n_grads (1..4) gradient buffers (`grads`: a host array of device pointers):
 *   g = sum * grad_scale + weight_decay*params;  exp_avg += (1-beta1)(g - exp_avg);
 *   exp_avg_sq = beta2*exp_avg_sq + (1-beta2) g*g;  t = step + 1;
 *   params -= lr/(1-beta1^t) * exp_avg / (sqrt(exp_avg_sq)/sqrt(1-beta2^t) + eps)
 * step: device float[1] = applied steps so far (torch's per-parameter `step`), advanced after the update; a skipped
 * step modifies none of params, moments, step and increments state[1].  hyper_device: double[6] on the device =
 * {lr, beta1, beta2, eps, weight_decay, grad_scale}, read when the kernels execute (a captured graph follows the
 * schedule).  Three launches: guard, update, a one-thread counter launch. */
int d3f_adam_guarded_step(const float* const* grads, int n_grads, float* params, float* exp_avg, float* exp_avg_sq,
                          float* step, size_t n, const double* hyper_device, int32_t* state, const int32_t* pair_status,
                          void* stream);
/* data-parallel form of the pair-status gate: poisons grad[0] with NaN before the exchange when the flag is set */
int d3f_poison_gradient_if_status(float* grad, const int32_t* pair_status, int32_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D3FEAT_HIP_H_ */
