/* openscene_amd.h -- C ABI of libopenscene_amd.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for ONE hot path of pengsongyou/openscene: hash voxelisation,
 * coordinate / kernel maps, sparse 3-D convolution (fwd, dgrad, wgrad), batch-norm
 * (+ReLU +residual), and the per-point feature x CLIP-text query.  Every entry
 * point names the reference interface it replaces (paths relative to the
 * reference tree; [ME] = NVIDIA/MinkowskiEngine v0.5.4, the un-vendored
 * dependency that holds the reference's arithmetic -- SURVEY.md appendix C).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch), unless the
 *     parameter is documented as "host";
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     except the few that return a count to the host (documented);
 *   - return value: 0 = OK, negative = error (OSN_E_*); text via osn_last_error()
 *     (thread-local); no C++ exception crosses the boundary;
 *   - the library allocates nothing: scratch comes in through `ws` arguments
 *     whose size the matching *_ws_bytes() helper reports;
 *   - callable from any host thread (autograd's backward thread included); no
 *     global mutable state.
 *   - feature matrices are row-major float32 [rows, channels]; coordinates are
 *     int32 rows (batch, x, y, z) exactly as the reference builds them
 *     (dataset/feature_loader.py:178-179,204-205).
 *   - a kernel map is a dense k-major neighbour table nbr[K, n_out] of int32,
 *     nbr[k, o] = input row found at coord[o] + offset_k, or -1.
 */
#ifndef OPENSCENE_AMD_H
#define OPENSCENE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSN_OK 0
#define OSN_E_ARG (-1)     /* bad argument (null pointer, size, alignment, range) */
#define OSN_E_HIP (-2)     /* a HIP runtime call or kernel launch failed          */
#define OSN_E_WS (-3)      /* workspace too small                                  */
#define OSN_E_RANGE (-4)   /* coordinate outside the packable range                */

typedef void* osn_stream_t; /* hipStream_t */

/* ---- library ------------------------------------------------------------- */
int osn_version(void);                 /* ABI version, bumped on any signature change */
const char* osn_last_error(void);      /* message of this thread's last failing call   */
int osn_device_ok(void);               /* 1 if the current HIP device is gfx950        */

/* ---- coordinate maps ----------------------------------------------------- *
 * Replaces [ME] CoordinateManager.insert_and_map / stride (called implicitly by
 *   SparseTensor(features, coordinates)   run/distill.py:316-317, run/evaluate.py:284
 *   stride-2 convolutions                 models/mink_unet.py:52-53,59-60,66-67,73-74).
 * The hash table is open addressing over a 64-bit packed key
 * (b<<48 | (x+2^15)<<32 | (y+2^15)<<16 | (z+2^15)); capacity = power of two.    */
int64_t osn_hash_capacity(int64_t n);                                  /* host helper */
size_t osn_coords_unique_ws_bytes(int64_t n);                          /* host helper */

/* Quantise rows to multiples of `stride` (floor; stride 1 = as is), de-duplicate.
 * out_coords4[u] = u-th distinct row in FIRST-OCCURRENCE order, inverse[i] = u,
 * first[u] = lowest input row of u.  On return the table (keys, vals) maps a packed
 * key to u and is what osn_kmap_build() probes.  *n_unique_host is written on the
 * HOST; the call synchronises `stream` once to deliver it.                      */
int osn_coords_unique(const int32_t* coords4, int64_t n, int stride,
                      uint64_t* table_keys, int32_t* table_vals, int64_t cap,
                      int32_t* out_coords4, int32_t* inverse, int32_t* first,
                      int64_t* n_unique_host, void* ws, size_t ws_bytes, osn_stream_t stream);

/* The same unique pipeline WITHOUT the host synchronisation, for chaining the levels of a coordinate pyramid
 * (models/mink_unet.py:52-74: four stride-2 levels are created per forward): everything is sized for n_max rows;
 * n_dev (nullable) = the actual row count in device memory (the previous level's count_dev), count_dev receives
 * this level's number of unique rows, err_dev is a sticky flag (zeroed by the caller) set on a coordinate outside
 * the packable range.  The caller reads all counts and the flag back ONCE.  Identical results to
 * osn_coords_unique on the first `count` rows.                                                                */
int osn_coords_unique_async(const int32_t* coords4, int64_t n_max, const int32_t* n_dev, int stride,
                            uint64_t* table_keys, int32_t* table_vals, int64_t cap, int32_t* out_coords4,
                            int32_t* inverse, int32_t* first, int32_t* count_dev, int32_t* err_dev,
                            void* ws, size_t ws_bytes, osn_stream_t stream);

/* The whole coordinate pyramid of a scene from ONE call (models/mink_unet.py:52-74: conv1p1s2 ... conv4p8s2 create four stride-2
 * levels below the input's): level i = the unique rows of level i - 1 quantised to strides[i], queued back to back with the row
 * counts in device memory -- osn_coords_unique_async per level, with one preset launch for all tables and counters and the flag pass
 * folded into the scan (31 instead of 45 dependent launches for five levels).  Every per-level array is sized for n0 rows / `cap`
 * slots; counts_dev[0 .. n_levels) receive the unique rows per level, counts_dev[n_levels] the sticky range-error flag (all zeroed
 * here); the caller reads them back ONCE.  Pointer arrays are HOST arrays of device pointers.  Results: bit for bit the per-level calls'. */
int osn_coords_pyramid_async(const int32_t* coords4, int64_t n0, const int32_t* strides, int n_levels,
                             uint64_t* const* table_keys, int32_t* const* table_vals, int64_t cap,
                             int32_t* const* out_coords4, int32_t* const* inverse, int32_t* const* first,
                             int32_t* counts_dev, void* ws, size_t ws_bytes, osn_stream_t stream);

/* Replaces [ME] CoordinateManager.kernel_map (HYPER_CUBE region).  Offsets
 * enumerate with x fastest; odd ksize centred, even ksize spans [0,ksize); all
 * multiplied by `offset_scale` (= dilation * tensor stride of the INPUT map).  */
int osn_kmap_build(const uint64_t* in_table_keys, const int32_t* in_table_vals, int64_t cap,
                   const int32_t* out_coords4, int64_t n_out, int ksize, int offset_scale,
                   int32_t* nbr, int64_t* counts /* nullable: int64 [K] pairs per offset */,
                   osn_stream_t stream);

/* The same map when the output coordinates ARE the table's own rows in row order (every stride-1
 * convolution of the path: models/mink_unet.py:47-113 BasicBlock convs, conv0p1s1) and ksize is odd:
 * such a map is its own mirror (nbr[k][o] = i <=> nbr[K-1-k][i] = o), so only the offsets below the centre
 * are probed and each hit also writes its mirrored entry.  Bit-identical output to osn_kmap_build. */
int osn_kmap_build_self(const uint64_t* table_keys, const int32_t* table_vals, int64_t cap,
                        const int32_t* coords4, int64_t n, int ksize, int offset_scale,
                        int32_t* nbr, int64_t* counts /* nullable */, osn_stream_t stream);

/* tbl[k, i] = o  <=>  nbr[k, o] = i : the map of the transposed operator
 * ([ME] MinkowskiConvolutionTranspose, models/mink_unet.py:77-78,84-85,91-92,98-99,
 * and the input-gradient of every strided convolution).                          */
int osn_kmap_transpose(const int32_t* nbr, int64_t n_out, int K, int64_t n_in, int32_t* tbl,
                       osn_stream_t stream);

/* Tile-order optimisation (no reference counterpart; ME's GPU kernels are unordered):
 * order[j] = output rows sorted (stably) by their offset-occupancy bit mask, and
 * nbr_sorted[k, j] = nbr[k, order[j]].  Feed both to osn_spconv_fwd (nbr_sorted as the
 * table, order as out_rows): rows of one tile then share their offsets and the per-tile
 * offset skip removes the empty work; results are unchanged.  K <= 32.
 * counts (nullable, int64 [K] = osn_kmap_count): orders the key bits by rarity (rarest offset = most
 * significant bit) instead of offset index, so the tiles that pay for a rare offset are few.        */
size_t osn_kmap_sort_ws_bytes(int64_t n_out);
int osn_kmap_sort(const int32_t* nbr, int64_t n_out, int K, const int64_t* counts, int32_t* order,
                  int32_t* nbr_sorted,
                  uint32_t* gmask /* nullable: uint32 [ceil(n_out/32)], OR of the occupancy masks of
                                     each 32-row group of the sorted table */,
                  void* ws, size_t ws_bytes, osn_stream_t stream);

/* counts[k] = #valid entries of nbr[k, :]  (int64 [K], device).                  */
int osn_kmap_count(const int32_t* nbr, int64_t n_out, int K, int64_t* counts, osn_stream_t stream);

/* ---- sparse convolution -------------------------------------------------- *
 * Replaces [ME] MinkowskiConvolution / MinkowskiConvolutionTranspose forward and
 * backward (constructed at models/mink_unet.py:47-113, models/resnet_base.py:92-97).
 *   out[o, :] = sum_k in[nbr[k, o], :] @ W[k]        W: [K, cin, cout] float32
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (bit-for-bit an fmaf chain).
 * out_rows (nullable): out row of tile slot j is out_rows[j] instead of j.       */
size_t osn_spconv_fwd_ws_bytes(int64_t n_out, int K, int cin, int cout);
int osn_spconv_fwd(const float* in, const float* W, const int32_t* nbr, const int32_t* out_rows,
                   const uint32_t* gmask /* nullable: osn_kmap_sort's group masks of `nbr`; lets the
                       kernel split each tile's ACTIVE offsets into equal work units (load balance) */,
                   float* out, int64_t n_out, int K, int cin, int cout,
                   void* ws, size_t ws_bytes, osn_stream_t stream);

/* Split-bf16 ("bf16x6") variant of osn_spconv_fwd: same result contract (fp32 in / fp32 out, fp32-level
 * accuracy: every operand is split into three bf16 pieces and the six significant cross products are
 * accumulated in fp32 on v_mfma_f32_32x32x16_bf16, 2.7x the fp32 MFMA throughput).  Wp comes from
 * osn_weight_prep_x6: bf16 [3][K][n_out_channels][c_padded]; for_dgrad = 1 prepares the (optionally
 * mirrored) transposed weights of the input gradient, replacing osn_weight_transpose.
 * Here `cin` = contraction channels of `in`, `cout` = output channels.  Needs cin % 4 == 0.          */
size_t osn_weight_prep_x6_bytes(int K, int cin, int cout, int for_dgrad);
int osn_weight_prep_x6(const float* W, int K, int cin, int cout, int flip, int for_dgrad, void* Wp,
                       osn_stream_t stream);
/* Both layouts of one weight in ONE launch (training: the forward planes now, the input-gradient planes
 * kept for the backward pass): Wp_fwd = prep(flip 0, for_dgrad 0), Wp_dgrad = prep(flip, for_dgrad 1). */
int osn_weight_prep_x6_pair(const float* W, int K, int cin, int cout, int flip, void* Wp_fwd, void* Wp_dgrad,
                            osn_stream_t stream);
int osn_spconv_fwd_x6(const float* in, const void* Wp, const int32_t* nbr, const int32_t* out_rows,
                      const uint32_t* gmask, float* out, int64_t n_out, int K, int cin, int cout,
                      void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- second-generation convolution: per-tile compacted pair lists ------------------------- *
 * Same result contract as osn_spconv_fwd / osn_spconv_fwd_x6 ([ME] MinkowskiConvolution[Transpose]
 * forward, models/mink_unet.py:47-113; fp32 in / fp32 out, split-bf16 arithmetic of fp32-class accuracy,
 * bitwise reproducible), other data layout: the kernel map of every tile of `bm` consecutive rows of a
 * neighbour table is stored per offset as a dense list of (input row, local output row) pairs -- what
 * [ME] calls the kernel map's in/out index lists, cut per tile -- so the matrix units only see real
 * pairs, the weights of an offset stay in registers for a whole (tile, offset), the output tile is
 * accumulated in LDS, and persistent workgroups draw the tiles from an atomic counter (densest first).
 *   osn_tile_rows(n_out)            rows per tile for a table of n_out rows (host helper, 32 .. 88)
 *   osn_tile_lists_build(nbr, ..)   tl = { int32 cnt[n_tiles][K] (256-byte aligned), int2 lst[n_tiles][K][bm] }
 *                                   from a (possibly osn_kmap_sort-ordered) table; lists keep row order
 *   osn_weight_prep_tl(W, ..)       MFMA-fragment images of a weight: Wp_fwd for the forward, Wp_dgrad
 *                                   (transposed, mirrored in k if flip) for the input gradient; either
 *                                   may be null; sizes from osn_weight_prep_tl_bytes
 *   osn_spconv_fwd_tl(..)           out[out_rows ? out_rows[j] : j] = sum_k in[list rows] @ W[k] for table
 *                                   row j; tl = null <=> K == 1 identity map.  bn_partial (nullable):
 *                                   double [n_tiles][2][cout] per-tile column sums / sums of squares of
 *                                   `out` (the following batch norm's statistics without a pass over out).
 *                                   ws: osn_spconv_fwd_tl_ws_bytes(..) bytes: a 512-byte head and, on
 *                                   small tables, the partial tiles of a launch that splits each tile's offsets over
 *                                   several workgroups (summed in a fixed order; bn_partial must be null there).
 *                                   counters (nullable): caller-owned PERSISTENT tile counters (128 int32 in device
 *                                   memory, zero before the first call, one buffer per stream): the kernel's last
 *                                   workgroup puts them back to zero, so the call needs no memset launch.  A launch
 *                                   that fails leaves them undefined (zero them again).  counters null: the tile
 *                                   counters are the head of ws, zeroed by the call.
 *                                   Needs cin % 4 == 0, cout % 4 == 0 and n_in <= 2^24 (OSN_E_RANGE otherwise).  */
int osn_tile_rows(int64_t n_out);
size_t osn_tile_lists_bytes(int64_t n_out, int K, int bm);
int osn_tile_lists_build(const int32_t* nbr, int64_t n_out, int K, int bm, void* tl, osn_stream_t stream);
size_t osn_weight_prep_tl_bytes(int K, int cin, int cout, int for_dgrad);
int osn_weight_prep_tl(const float* W, int K, int cin, int cout, int flip, void* Wp_fwd, void* Wp_dgrad,
                       osn_stream_t stream);
size_t osn_spconv_fwd_tl_ws_bytes(int64_t n_out, int K, int cout, int bm);
int osn_spconv_fwd_tl(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows,
                      float* out, double* bn_partial, int64_t n_out, int K, int cin, int cout, int bm,
                      void* ws, size_t ws_bytes, int32_t* counters, osn_stream_t stream);

/* ---- reduced-precision inference: the `_pieces` siblings of the four split-bf16 forward entries ---------------------- *
 * (function parity with the inference call sites of the reference, which round the network's output to fp16 at once:
 * run/evaluate.py:290-292; the convolutions are those of models/mink_unet.py:47-113 and models/resnet_base.py:38-60, 101-107,
 * as cited at each base entry.)  Each sibling takes the arguments of its base entry plus a trailing `int pieces`:
 *     pieces   name     operand pieces   products h_i(a) h_j(b) kept, in accumulation order (smallest first)
 *       3      bf16x6   h1 h2 h3         31 22 13 21 12 11      -- bit for bit the base entry, which calls the same code with 3
 *       2      bf16x3   h1 h2            21 12 11
 *       1      bf16x1   h1               11                     -- one round-to-nearest bf16 per operand
 * i.e. "ij" is kept iff i + j <= pieces + 1.  fp32 accumulation, fixed summation order, bitwise repeatable, in every mode.
 * A reduced launch reads planes 0 .. pieces - 1 of the SAME weight image (osn_weight_prep_tl): no other layout, nothing to prepare.
 * Error against the exact value, per output element and in units of sum_k |a_k||b_k| (on top of the half ulp of the result):
 * 2e-6 (pieces 3), 2^-15 + 2e-6 (pieces 2), 2^-7 + 2e-6 (pieces 1); against the float64 sum of the kept products of the exact
 * pieces 2e-6 in every mode (tests/conv_pieces.py).  pieces outside {1, 2, 3}: OSN_E_ARG before anything else is looked at.
 * Forward inference only: weight gradients, the stem (osn_stem_conv_fwd) and the first-generation kernels have no reduced mode; an
 * input gradient may be computed through a sibling (it is the same launch on the other weight image) but the library never does.
 * Every shape of a base entry has reduced instances, except: osn_spconv_fwd_tl_pieces on a feature matrix of 2 GB or more (or of
 * exactly 2^24 rows) whose input channels fill whole chunks (cin % 32 == 0 and cin / 32 <= 4 or divisible by 4 or 3) runs the
 * six-product kernel for every `pieces` -- more exact than asked, never an error.                                          */
int osn_spconv_fwd_tl_pieces(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows,
                             float* out, double* bn_partial, int64_t n_out, int K, int cin, int cout, int bm,
                             void* ws, size_t ws_bytes, int32_t* counters, osn_stream_t stream, int pieces);
int osn_dense_fwd_pieces(const float* in, const void* Wp, float* out, int64_t n, int cin, int cout, osn_stream_t stream,
                         int pieces);
int osn_spconv_fwd_rg_pieces(const float* in, int64_t n_in, const void* Wp, const int32_t* nbr, const int32_t* out_rows,
                             float* out, int64_t n_out, int K, int cin, int cout, osn_stream_t stream, int pieces);
int osn_spconv_fwd_ws_pieces(const float* in, int64_t n_in, const void* Wp, const void* pl, int64_t pl_rows, int swap,
                             int direct, const int32_t* nbr_dst, float* out, int64_t n_dst, int K, int cin, int cout,
                             void* ws, size_t ws_bytes, osn_stream_t stream, int pieces);

/* ---- every weight image of a model in one launch ----------------------------------------------- *
 * [ME] keeps one `kernel` parameter per MinkowskiConvolution / MinkowskiConvolutionTranspose
 * (models/mink_unet.py:47-113, models/resnet_base.py:38-60); an optimizer step changes all of them at once.
 * Instead of one osn_weight_prep_x6 / osn_weight_prep_tl launch per convolution and step, the host keeps a
 * table of jobs in DEVICE memory (built once per model: pointers and shapes do not change) and one launch
 * fills every image.  jobs[i].first_block = sum of osn_weight_prep_job_blocks(...) of the jobs before i,
 * total_blocks = the sum over all jobs.  Image contents are identical to the per-weight entry points
 * (layout OSN_PREP_X6: osn_weight_prep_x6(W, .., flip, for_dgrad); OSN_PREP_TL: the Wp_fwd (for_dgrad = 0)
 * or Wp_dgrad (for_dgrad = 1) of osn_weight_prep_tl).                                                      */
enum { OSN_PREP_X6 = 0, OSN_PREP_TL = 1 };
typedef struct osn_prep_job {
    const float* W;       /* [K][cin][cout] fp32 weight                                   */
    void* out;            /* image: osn_weight_prep_x6_bytes / osn_weight_prep_tl_bytes    */
    int64_t first_block;  /* exclusive prefix of the jobs' block counts                    */
    int32_t K, cin, cout; /* weight shape                                                  */
    int32_t flip;         /* mirror the offsets (input gradient of stride-1 odd kernels)   */
    int32_t for_dgrad;    /* 1: image of the transposed weight                             */
    int32_t layout;       /* OSN_PREP_X6 | OSN_PREP_TL                                     */
} osn_prep_job;           /* 48 bytes */
int64_t osn_weight_prep_job_blocks(int K, int cin, int cout, int for_dgrad, int layout);
int osn_weight_prep_batch(const osn_prep_job* jobs_dev, int n_jobs, int64_t total_blocks, osn_stream_t stream);

/* Which kernel instance / launch shape osn_spconv_fwd() uses for a problem (host helper, for
 * profiling): plan6 = {WM, WN, TN, BK, S (offset splits), workgroups};
 * the kernel symbol is spconv_fwd_kernel<WM, WN, TN, BK>.                          */
int osn_spconv_fwd_plan(int64_t n_out, int K, int cin, int cout, int32_t* plan6);

/* The shapes each convolution kernel family is ROUTED to: 1 or 0, pure host arithmetic (no device, no launch, no error string;
 * 0 for non-positive sizes).  Each is defined beside its kernel and is the one statement of that kernel's limits: the executor
 * (csrc/net.hip) and openscene_amd.ops ask these.  An entry point may accept more than its predicate (4 input channels,
 * K == 1); osn_spconv_fwd_rg_ok, further down, is the fifth.                                                              */
/* stem.hip: cin <= 4, cout == 32, 1 < K <= 125 */
int osn_stem_conv_ok(int K, int cin, int cout);
/* spconv_tl.hip: cin % 4 == 0 in [8, 512] (the step table's four 128-channel chunks), cout % 4 == 0, K <= 128, n_in <= 2^24 (0 allowed) */
int osn_spconv_fwd_tl_ok(int64_t n_in, int K, int cin, int cout);
/* dense.hip: cin % 4 == 0, cin >= 8, cout % 4 == 0 */
int osn_dense_fwd_ok(int cin, int cout);
/* spconv.hip (split-bf16): cin % 4 == 0, cin >= 8, a weight image within 32-bit offsets, at most 32 offsets per block of the launch plan for n_out rows (<= 0: 1) */
int osn_spconv_fwd_x6_ok(int64_t n_out, int K, int cin, int cout);

/* Wt[k] = W[flip ? K-1-k : k]^T   ([K, cout, cin]).  The input gradient is
 * osn_spconv_fwd(gout, Wt, table, ...) with table = nbr and flip = 1 for a
 * stride-1 odd kernel (the map is its own mirror), or the transposed table and
 * flip = 0 otherwise.                                                             */
int osn_weight_transpose(const float* W, int K, int cin, int cout, int flip, float* Wt,
                         osn_stream_t stream);

/* gW[k] = sum_{o : nbr[k,o] >= 0} in[nbr[k,o], :]^T (x) gout[o, :]   ([K, cin, cout]).
 * counts (nullable, device int64 [K], = osn_kmap_count of nbr): pair count per offset, used
 * to split each offset's rows into work items of equal pair count on the device (the centre
 * offset of a 3^3 map holds 19 % of the pairs, a corner offset < 1 %).  Deterministic: the
 * split is a pure function of (counts, sizes); partial sums are reduced in item order.
 * plan_items (nullable): the work-item table osn_spconv_wgrad_plan() wrote for the same
 * (counts, n_out, K) and a (cin, cout) with the same osn_spconv_wgrad_items_bytes -- the table
 * depends on the map only, so the convs of one map share it and skip the per-call plan launch. */
size_t osn_spconv_wgrad_ws_bytes(int64_t n_out, int K, int cin, int cout);
size_t osn_spconv_wgrad_items_bytes(int64_t n_out, int K, int cin, int cout);
int osn_spconv_wgrad_plan(const int64_t* counts, int64_t n_out, int K, int cin, int cout,
                          int32_t* items /* osn_spconv_wgrad_items_bytes */, osn_stream_t stream);
int osn_spconv_wgrad(const float* in, const float* gout, const int32_t* nbr, const int64_t* counts,
                     const int32_t* plan_items, float* gW, int64_t n_out, int K, int cin, int cout,
                     void* ws, size_t ws_bytes, osn_stream_t stream);

/* Second-generation weight gradient: the pairs of every offset compacted ONCE per map into arrays
 * (input row, output row) in tile order -- [ME]'s kernel-map in/out index lists -- shared by every
 * convolution and every step of the map's life; split-bf16 arithmetic on the bf16 MFMA with LDS transpose
 * reads (fp32-class accuracy, bitwise reproducible: work items are a pure function of the map, partial sums
 * are reduced in item order).
 *   osn_pair_lists_build(tl, ..)    pl = per-offset pair arrays + device-planned work items, from the tile
 *                                   lists `tl` of a table with n_out rows (bm as given to osn_tile_lists_build;
 *                                   out_rows = the table's row permutation or null); osn_pair_lists_bytes
 *   osn_spconv_wgrad_tl(..)         gW[k] = sum over the pairs of offset k of in[i]^T (x) gout[o]  ([K, cin, cout]).
 *                                   swap = 1: the arrays belong to the strided convolution this TRANSPOSED
 *                                   convolution mirrors (in rows are indexed by the arrays' output rows).
 *                                   pl = null <=> K == 1 identity map.  Needs cin % 4 == 0 and cout % 4 == 0.   */
size_t osn_pair_lists_bytes(int64_t n_out, int K, int bm);
int osn_pair_lists_build(const void* tl, const int32_t* out_rows, int64_t n_out, int K, int bm, void* pl,
                         osn_stream_t stream);
size_t osn_spconv_wgrad_tl_ws_bytes(int K, int cin, int cout);
int osn_spconv_wgrad_tl(const float* in, const float* gout, const void* pl, int swap, float* gW, int64_t n_in,
                        int64_t n_out, int K, int cin, int cout, void* ws, size_t ws_bytes, osn_stream_t stream);

/* The two halves of osn_spconv_wgrad_tl for callers that run many weight gradients back to back (the network executor):
 * osn_spconv_wgrad_tl_partial launches the kernel only -- partial sums per work item into `partial`
 * (osn_spconv_wgrad_tl_ws_bytes bytes, must stay untouched until the reduction ran) -- and fills `job` (HOST);
 * osn_wgrad_tl_reduce_batch reduces any number of such jobs in ONE launch per 32 jobs (same summation order as
 * osn_spconv_wgrad_tl: bitwise the same gradient).  A job whose gW is null (empty map: gW was zeroed) is skipped.  */
typedef struct osn_wgrad_job {
    const float* partial;        /* device */
    const void* range;           /* device: items of each offset, or null (identity map: items [0, ident_items))     */
    float* gW;                   /* device, [K, cin, cout]                                                         */
    int32_t K, cin, cout, ident_items;
} osn_wgrad_job;                 /* 40 bytes */
int osn_spconv_wgrad_tl_partial(const float* in, const float* gout, const void* pl, int swap, float* gW, int64_t n_in,
                                int64_t n_out, int K, int cin, int cout, void* partial, size_t partial_bytes,
                                osn_wgrad_job* job_host, osn_stream_t stream);
int osn_wgrad_tl_reduce_batch(const osn_wgrad_job* jobs_host, int n_jobs, osn_stream_t stream);

/* ---- reduced-precision training: the `_pieces` siblings of the two weight-gradient entries -------------------------------- *
 * The arguments of the base entry plus a trailing `int pieces`, with the meaning of the `_pieces` forward entries above: both
 * operands (gathered input rows, gathered output-gradient rows) are split into `pieces` bf16 pieces and "ij" is kept iff
 * i + j <= pieces + 1, in the same accumulation order; the per-item partial sums stay fp32 and are reduced in item order by the
 * same launches (osn_wgrad_tl_reduce_batch takes the jobs of every mode), so the result is bitwise repeatable in every mode and
 * partial + batched reduction is bitwise the one-call entry.  pieces == 3 is bitwise the base entry.  Error per element of gW, in
 * units of the sum over the offset's pairs of |in||gout|: fp32-class (pieces 3), 2^-15 more (pieces 2), 2^-7 more (pieces 1);
 * against the float64 sum of the kept products of the exact pieces fp32-class in every mode (tests/train_pieces.py).
 * pieces outside {1, 2, 3}: OSN_E_ARG before anything else is looked at.  Every shape of the base entries has reduced instances
 * (all <MB, NB> blockings, identity maps, swap, strided items, both addressing modes): none falls back to three pieces.  Workspace
 * and job layout are those of the base entries (osn_spconv_wgrad_tl_ws_bytes).  The first-generation osn_spconv_wgrad and the
 * stem's weight gradient have no reduced mode.                                                                              */
int osn_spconv_wgrad_tl_pieces(const float* in, const float* gout, const void* pl, int swap, float* gW, int64_t n_in,
                               int64_t n_out, int K, int cin, int cout, void* ws, size_t ws_bytes, osn_stream_t stream,
                               int pieces);
int osn_spconv_wgrad_tl_partial_pieces(const float* in, const float* gout, const void* pl, int swap, float* gW, int64_t n_in,
                                       int64_t n_out, int K, int cin, int cout, void* partial, size_t partial_bytes,
                                       osn_wgrad_job* job_host, osn_stream_t stream, int pieces);

/* 1x1 convolution = row-wise matrix product ([ME] MinkowskiConvolution(kernel_size=1): the head `final`,
 * models/mink_unet.py:108-113, and the BasicBlock shortcuts, models/resnet_base.py:101-107; with the input-gradient image
 * their backward):  out[n, cout] = in[n, cin] @ B,  B given as an osn_weight_prep_tl image with K = 1 (forward image:
 * B = W; input-gradient image: B = W^T, `cin` then counts the conv's OUTPUT channels).  Same split-bf16 arithmetic as
 * osn_spconv_fwd_tl; no workspace.  Needs cin % 4 == 0, cin >= 8, cout % 4 == 0.                                    */
int osn_dense_fwd(const float* in, const void* Wp, float* out, int64_t n, int cin, int cout, osn_stream_t stream);

/* Convolution of a NARROW layer (32 or 64 channels on both sides) straight from the neighbour table ([ME]
 * MinkowskiConvolution forward, models/mink_unet.py:59-93: conv1p1s2 .. block2 -- the 32- and 64-channel stages of the encoder --
 * and, with the input-gradient image and the mirrored table, their backward): every lane of a wave gathers the 32 bytes of the
 * fp32 row that ARE its MFMA operand (two 16-byte loads through nbr; an absent neighbour reads zeros and moves no data), splits
 * them in registers and multiplies -- no staging through LDS, no barrier in the loop.  A workgroup owns 64 table rows, its four
 * waves take the offsets w, w + 4, ..., partial tiles are summed in wave order (bitwise reproducible).  Same arithmetic and
 * weight image as osn_spconv_fwd_tl (osn_weight_prep_tl).  nbr: int32 [K, n_out], plain or osn_kmap_sort-ordered (then out_rows =
 * its permutation: table row j is written to out[out_rows[j]]).  osn_spconv_fwd_rg_ok: 1 for the shapes it takes (K > 1, cin and
 * cout in {32, 64}, n_in < 2^24, the feature matrix below 2 GB).                                                           */
int osn_spconv_fwd_rg_ok(int64_t n_in, int K, int cin, int cout);
int osn_spconv_fwd_rg(const float* in, int64_t n_in, const void* Wp, const int32_t* nbr, const int32_t* out_rows, float* out,
                      int64_t n_out, int K, int cin, int cout, osn_stream_t stream);

/* Convolution of a SMALL map (<= 16 k rows) from its per-offset pair arrays, weight-stationary ([ME]
 * MinkowskiConvolution[Transpose] forward, models/mink_unet.py:51-113 on the 1/4 .. 1/16 levels; with the input-gradient
 * weight image also their backward):  a workgroup keeps W[k] of ONE offset in registers and multiplies a chunk of that
 * offset's pairs, writes the result rows to partial[k][dst row]; a second launch sums out[r] over the offsets k the
 * destination table has at r, ascending (fixed order, bitwise reproducible).  Same arithmetic and weight images as
 * osn_spconv_fwd_tl (osn_weight_prep_tl: forward image, or the input-gradient image for a backward launch).
 *   pl / pl_rows  pair arrays (osn_pair_lists_build) of a map with pl_rows output rows;
 *   swap = 0      gathers pin -> writes pout: the map's own direction (pl_rows == n_dst);
 *   swap = 1      gathers pout -> writes pin: the transposed direction (pl_rows == n_in) -- input gradient of a strided
 *                 convolution, forward of the transposed convolution that mirrors it;
 *   nbr_dst       int32 [K, n_dst] neighbour table of the DESTINATION side in plain row order (>= 0 <=> partial[k][r] was
 *                 written): nbr_fwd for swap = 0, the transposed table (osn_kmap_transpose) for swap = 1.
 *   direct = 1    the caller guarantees that every destination row has EXACTLY ONE pair in the whole map -- the fine side
 *                 of a 2^3 stride-2 map (a voxel has one parent cell): forward of [ME] MinkowskiConvolutionTranspose
 *                 (kernel 2, stride 2) and input gradient of the strided convolution.  The result rows then go straight to
 *                 `out`: no partial rows, no second launch, any map size; nbr_dst may be null.
 * ws: osn_spconv_fwd_ws_ws_bytes(n_dst, K, cout, direct) bytes (the partial rows).  Needs 2 <= K <= 128,
 * cin % 4 == cout % 4 == 0. */
size_t osn_spconv_fwd_ws_ws_bytes(int64_t n_dst, int K, int cout, int direct);
int osn_spconv_fwd_ws(const float* in, int64_t n_in, const void* Wp, const void* pl, int64_t pl_rows, int swap, int direct,
                      const int32_t* nbr_dst, float* out, int64_t n_dst, int K, int cin, int cout, void* ws,
                      size_t ws_bytes, osn_stream_t stream);

/* The 3-channel stem convolution (conv0p1s1: 5^3 kernel, 3 -> 32, models/mink_unet.py:47-50): same contract as
 * osn_spconv_fwd on the plain (unordered) table, for cin <= 4 and cout == 32.  Below 32 768 output rows: exact fp32 FMA
 * chains in ascending offset order.  From 32 768 rows on (round 6): a matrix product on the MFMA units -- two table entries
 * x four padded channels per lane, the library's split-bf16 arithmetic (fp32-class: three bf16 pieces per operand, six
 * products, fp32 accumulate), partial tiles of four waves summed in wave order.  Bitwise reproducible either way.           */
int osn_stem_conv_fwd(const float* in, const float* W, const int32_t* nbr, float* out, int64_t n_out, int K,
                      int cin, int cout, osn_stream_t stream);
/* Its weight gradient gW[k][ci][n] = sum_o in[nbr[k][o]][ci] * gout[o][n] ([ME] MinkowskiConvolutionFunction backward for
 * the same layer): dense over the table (an absent neighbour is a zero row), rows in ascending order, per-workgroup partial
 * sums added in a fixed order -- bitwise reproducible.  Below 32 768 rows fp32 fmaf chains; from 32 768 rows on the
 * contraction over the rows runs on the MFMA units (split-bf16, 32 rows per step, one accumulator set per input channel,
 * 512 partial gradients).  ws: osn_stem_conv_wgrad_ws_bytes.                                                                */
size_t osn_stem_conv_wgrad_ws_bytes(int K, int cin);
int osn_stem_conv_wgrad(const float* in, const float* gout, const int32_t* nbr, float* gW, int64_t n_out, int K, int cin,
                        int cout, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- batch norm (+ReLU, +residual) -------------------------------------- *
 * Replaces [ME] MinkowskiBatchNorm (= torch.nn.BatchNorm1d on .F), MinkowskiReLU
 * and the BasicBlock residual add (models/mink_unet.py:50-114, resnet_base.py:98).
 * Training statistics: biased variance for normalisation, unbiased for the
 * running estimate, momentum as torch.                                            */
size_t osn_bn_ws_bytes(int64_t n, int c);
/* mean[c], var[c] (biased) of x; if running_mean/var non-null update them in place:
 * r = (1-momentum) r + momentum * stat  (var unbiased).                           */
int osn_bn_stats(const float* x, int64_t n, int c, float* mean, float* var,
                 float* running_mean, float* running_var, float momentum,
                 void* ws, size_t ws_bytes, osn_stream_t stream);
/* y = act( (x - mean) * rsqrt(var + eps) * gamma + beta  [+ residual] ),  act = ReLU if relu.
 * y2 (nullable; ld2 is then not read) is a SECOND destination: the same rows also stored as a column window of a wider
 * matrix (y2 = first element of the window, ld2 = that matrix's row stride in floats, >= c and % 4 == 0) -- ME.cat
 * (models/mink_unet.py:147,155,163,171) written in place by the producers of its two halves.                        */
int osn_bn_apply(const float* x, const float* mean, const float* var, const float* gamma,
                 const float* beta, float eps, const float* residual, int relu, float* y,
                 float* y2, int64_t ld2, int64_t n, int c, osn_stream_t stream);
/* osn_bn_stats + osn_bn_apply in one call (training-mode forward of MinkowskiBatchNorm [+ residual] [+ MinkowskiReLU],
 * models/mink_unet.py:116-174; mean / var are outputs kept for the backward; y2 / ld2 as in osn_bn_apply).  Maps of at
 * most 4096 rows (the deep U-Net levels) run as ONE launch (statistics and apply from registers).                    */
int osn_bn_forward_train(const float* x, int64_t n, int c, const float* gamma, const float* beta, float eps,
                         const float* residual, int relu, float momentum, float* mean, float* var,
                         float* running_mean, float* running_var, float* y, float* y2, int64_t ld2,
                         void* ws, size_t ws_bytes, osn_stream_t stream);
/* Backward of osn_bn_apply.  g = relu ? gy * (y > 0) : gy.
 * training != 0 (batch statistics were used):
 *   gx = gamma * invstd * (g - mean_rows(g) - xhat * mean_rows(g * xhat))
 * training == 0 (running statistics): gx = gamma * invstd * g.
 * ggamma = sum_rows(g * xhat), gbeta = sum_rows(g); gres (nullable) = g.
 * gy, the incoming gradient, is the SUM of n_gy (1..3) row-aligned matrices, each with its own row stride (HOST arrays
 * of device pointers / strides in floats, >= c and % 4 == 0): a block input feeds conv1 and the residual, an encoder
 * output feeds the next stride-2 convolution and -- through ME.cat -- two convolutions of the decoder
 * (models/mink_unet.py:116-174); the sum autograd would form with separate add kernels is formed while reading.
 * beta (nullable): for a batch norm + ReLU WITHOUT a residual, y may be null when beta is given -- the mask (y > 0) is
 * recomputed from x with the forward pass's own expression, so neither backward pass reads y (models/resnet_base.py:98:
 * bn -> relu).  relu with neither y nor beta, or a null y together with gres, is OSN_E_ARG.
 * gres (a batch norm with a residual): the column-sum pass stores g = the masked sum of the sources to gres and the apply pass
 * reads it back instead of forming it a second time from y and the sources.  ALIASING RULE: that data flow is used only when
 * gres [n, c] overlaps none of x, y, gx and the gradient sources (each source's range is (n - 1) * ld + c floats); a gres that
 * overlaps any of them (e.g. gres written in place over source 0) takes the earlier flow, in which both passes form g and
 * the apply pass writes gres element by element.  Every output is bit for bit the same on both flows.                    */
int osn_bn_backward(const float* x, const float* y, const float* const* gy_host, const int64_t* gy_ld_host, int n_gy,
                    const float* mean, const float* var, const float* gamma, const float* beta, float eps, int relu,
                    int training, float* gx, float* gres, float* ggamma, float* gbeta, int64_t n, int c, void* ws,
                    size_t ws_bytes, osn_stream_t stream);

/* The launch plan of the apply kernels (osn_bn_apply, the apply pass of osn_bn_backward) for total4 = n * c / 4 quads of
 * c4 = c / 4 column quads: *grid = workgroups of 256 threads.  *flat = 0: grid * 256 is a multiple of c4 -- the smallest such grid
 * >= min(2048, ceil(total4 / 256)), at most 127 above it -- and every thread keeps its column quad (per-column constants and the
 * four 1 / sqrt(var + eps) taken once per thread).  *flat = 1: no such grid (wide odd c4); the flat kernels, which take column and
 * constants again for every quad, run on min(2048, ceil(total4 / 256)) workgroups.  Host only, no device needed.            */
int osn_bn_apply_plan(int64_t total4, int c4, int* grid, int* flat);
/* Tests and A/B only, process-wide: on != 0 runs the batch-norm kernels of the earlier rounds -- the flat apply kernels whatever
 * the plan says, and column sums with one row in flight per thread.  Every result is bit for bit the same either way.
 * Returns the previous setting.                                                                                              */
int osn_bn_set_flat_kernels(int on);
/* With batch statistics, the backward pass of a map of at most 64 row blocks of column sums (n <= 4096 rows), of any width,
 * runs in TWO launches: the apply pass works in groups of 32 columns, every workgroup adds the row blocks' partial sums of its
 * columns itself, in the order of the finalize kernel, and the workgroups of the first 32 rows write ggamma and gbeta.  Tests
 * and A/B only, process-wide: on != 0 keeps the finalize kernel a launch of its own on every map (as evaluation mode and
 * osn_bn_set_flat_kernels(1) do).  Every result is bit for bit the same either way.  Returns the previous setting.          */
int osn_bn_set_separate_finalize(int on);

/* ---- distillation loss on the supervised rows ------------------------------- *
 * Replaces run/distill.py:322-328 and its autograd chain:
 *     output_3d = output_3d[mask]
 *     loss = (1 - torch.nn.CosineSimilarity()(output_3d, feat_3d)).mean()      kind 0 ('cosine')
 *     loss = torch.nn.L1Loss()(output_3d, feat_3d)                             kind 1 ('l1')
 *   out     float [n, d]       the network output, input row order
 *   sel     int64 [n_sel]      rows the loss sees (= mask.nonzero(): distinct, any order), target[j] belongs to out[sel[j]]
 *   target  float [n_sel, d]   feat_3d
 *   loss    float [1]  (device)
 *   state   osn_distill_loss_state_bytes(n, n_sel) bytes kept by the caller from the forward to the backward call
 *   gloss   float [1] (device) gradient of the loss, or null (= 1)
 *   gout    float [n, d]       receives d loss / d out: the closed-form row gradient on the selected rows, ZEROS elsewhere
 *                              (what autograd's index backward produces with an index_add into a zero-filled tensor)
 * osn_distill_loss_check synchronises the stream and reports an index outside [0, n) or a row selected twice
 * (OSN_E_ARG); the kernels themselves never read or write out of bounds.  d % 4 == 0.                          */
size_t osn_distill_loss_state_bytes(int64_t n, int64_t n_sel);
int osn_distill_loss_fwd(const float* out, const int64_t* sel, const float* target, int64_t n, int64_t n_sel, int d, int kind,
                         float* loss, void* state, size_t state_bytes, osn_stream_t stream);
/* grows (nullable): additionally grows[j, :] = gout[sel[j], :], the non-zero rows of the gradient once more, compacted,
 * for osn_net_run.goutput_rows (the first n int32 of `state` are osn_net_run.grows_pos)                                  */
int osn_distill_loss_bwd(const float* out, const float* target, const float* gloss, int64_t n, int64_t n_sel, int d, int kind,
                         float* gout, float* grows, const void* state, size_t state_bytes, osn_stream_t stream);
int osn_distill_loss_check(const void* state, int64_t n, int64_t n_sel, osn_stream_t stream);

/* ---- optimizer step over one flat buffer ------------------------------------------------------------ *
 * Replaces optimizer.step() of torch.optim.Adam (run/distill.py:170-178 builds it, :333 steps it) for parameters,
 * gradients and moment estimates laid out as four flat fp32 arrays of n elements (n % 4 == 0; the network executor's
 * gradient buffer has that layout).  step = the 1-based count of this update.  The update rule of torch's Adam
 * (amsgrad = False, maximize = False; L2 weight decay added to the gradient): one launch, 28 bytes per parameter.   */
int osn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step, float lr,
                  float beta1, float beta2, float eps, float weight_decay, osn_stream_t stream);

/* SGD with momentum over the same flat layout.  Replaces optimizer.step() of torch.optim.SGD(model.parameters(), lr,
 * momentum, weight_decay) (run/train_mink.py:147-148 builds it, :283 steps it; its lr is set per iteration, :303-306).
 * torch's update rule (maximize = False):  d = g + weight_decay p;  momentum_buf = first ? d : momentum momentum_buf +
 * (1 - dampening) d;  d = nesterov ? d + momentum momentum_buf : momentum_buf;  p -= lr d.  `first` = the buffer does not
 * exist yet (torch's `momentum_buffer is None`); with momentum == 0 there is no buffer and momentum_buf may be null.
 * n % 4 == 0, 16-byte aligned arrays: one launch, 20 bytes per parameter (12 without momentum).                      */
int osn_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                 float weight_decay, int nesterov, int first, osn_stream_t stream);

/* ---- supervised segmentation head: cross-entropy, argmax, confusion matrix, test-repeat votes -------------- *
 * Replaces the supervised baseline's per-iteration head (run/train_mink.py:160,279-290,367-372):
 *     loss = nn.CrossEntropyLoss(ignore_index=255)(output, label)
 *     output = output.detach().max(1)[1]
 *     intersection, union, target = intersectionAndUnionGPU(output, label, classes, 255)   (util/util.py:132-145)
 * the numpy confusion matrix of util/metric.py:9-25 and the vote over test repeats of run/eval_mink.py:184-216.
 *   logits     float [n, c]  (1 <= c <= 256, any c: rows need no alignment)
 *   rows       int64 [n_lab] or null: row j of the head reads logits[rows[j]] (output[inds_reverse]); null: n_lab == n
 *   labels     int64 [n_lab]; rows whose label == ignore_index (255, or torch's -100) count in neither loss nor confusion
 *   loss       float [1] (device, nullable) = sum over labelled rows of (logsumexp(x) - x[y]) / n_valid; NaN if n_valid == 0.
 *              A fixed-order two-level sum (per-workgroup fp64 partials, then a one-workgroup launch): bitwise reproducible
 *   pred       int64 [n_lab] (nullable) = torch.max(x, 1)[1] (lowest column on a tie)
 *   confusion  int64 [c, c] (nullable), ACCUMULATED: confusion[pred * c + label] += 1 over the labelled rows.  diag =
 *              intersection, row sums = output, column sums = target of intersectionAndUnionGPU
 *   state      osn_seg_loss_state_bytes(n_lab, c) bytes kept by the caller from the forward to the backward call
 * osn_seg_loss_bwd (rows == null only): glogits [n, c] = gloss (softmax(x) - onehot(y)) / n_valid on labelled rows, zeros
 * on the others (gloss float [1] on the device, null = 1).  osn_seg_loss_check synchronises the stream and reports a label
 * outside [0, c) that is not ignore_index, or a rows entry outside [0, n) (OSN_E_ARG); the kernels never read or write out of
 * bounds (such a row counts as ignored).  osn_seg_vote: votes [n_pts, c] += logits[rows ? rows[p] : p] (a rows entry outside
 * [0, n) adds nothing); the vote's argmax and confusion then come from osn_seg_loss_fwd on `votes` with loss = null.     */
size_t osn_seg_loss_state_bytes(int64_t n_lab, int c);
int osn_seg_loss_fwd(const float* logits, const int64_t* rows, const int64_t* labels, int64_t n, int64_t n_lab, int c,
                     int64_t ignore_index, float* loss, int64_t* pred, int64_t* confusion, void* state, size_t state_bytes,
                     osn_stream_t stream);
int osn_seg_loss_bwd(const float* logits, const int64_t* labels, const float* gloss, int64_t n, int c, int64_t ignore_index,
                     float* glogits, const void* state, size_t state_bytes, osn_stream_t stream);
int osn_seg_loss_check(const void* state, int64_t n, int64_t n_lab, int c, osn_stream_t stream);
int osn_seg_vote(const float* logits, const int64_t* rows, int64_t n, int64_t n_pts, int c, float* votes, osn_stream_t stream);

/* ---- row-aligned elementwise pieces --------------------------------------- *
 * Replaces the stand-alone [ME] MinkowskiReLU (models/mink_unet.py:114, used un-fused by the reference's own module
 * chain), the BasicBlock residual `out += residual` when it is not fused into a batch norm, and ME.cat of two tensors
 * on one coordinate map (models/mink_unet.py:147,155,163,171) with its backward split.  `total` = rows x channels.
 *   osn_relu_fwd   y = max(x, 0)                       osn_relu_bwd   gx = y > 0 ? gy : 0
 *   osn_add        out = a + b  (out may alias a or b)
 *   osn_cat2       out[r] = (a[r, 0:ca], b[r, 0:cb])   osn_cat2_bwd   ga[r] = gout[r, 0:ca], gb[r] = gout[r, ca:ca+cb]
 * cat: ca and cb multiples of 4 (every width of the MinkUNet family is).                                          */
int osn_relu_fwd(const float* x, float* y, int64_t total, osn_stream_t stream);
int osn_relu_bwd(const float* y, const float* gy, float* gx, int64_t total, osn_stream_t stream);
int osn_add(const float* a, const float* b, float* out, int64_t total, osn_stream_t stream);
int osn_cat2(const float* a, int ca, const float* b, int cb, float* out, int64_t n, osn_stream_t stream);
int osn_cat2_bwd(const float* gout, float* ga, int ca, float* gb, int cb, int64_t n, osn_stream_t stream);

/* ---- open-vocabulary query ---------------------------------------------- *
 * Replaces run/evaluate.py:290-292 (and run/distill.py:423-425):
 *   pred = feats[inds_reverse].half() @ text.t();  label = argmax(pred, 1)
 * X float32 [n_rows_x, d]; gather (nullable) int64 [n]; text fp16 [c, d];
 * scores (nullable) fp16 [n, c]; argmax int64 [n].  fp16 MFMA, fp32 accumulate,
 * one rounding to fp16.  The contract (tests/query_bounds.py holds every kernel to it):
 *   Scores.  xh = fp16_rne(x) is the reference's .half() (overflow becomes +-inf);
 *   S = sum_k xh_k t_k and A = sum_k |xh_k| |t_k| in float64.  Every fp16 score satisfies
 *       fp16_rne(S - c A)  <=  score  <=  fp16_rne(S + c A),      c = 2e-6,
 *   float64 rounded to fp16 in one step; where the two ends are +-inf or NaN the score
 *   is that value.
 *   Labels.  label = torch.max(scores, 1)[1] of the kernel's OWN fp16 scores on every
 *   row: the first NaN wins, otherwise the lowest column among equal maxima
 *   (-0.0 == +0.0); the same label with and without the score matrix.
 * osn_rows_argmax obeys the same label rule on its float32 scores.                   */
int osn_cosine_query(const float* X, const int64_t* gather, const void* text_f16,
                     void* scores_f16, int64_t* argmax, int64_t n, int d, int c,
                     osn_stream_t stream);
/* run/evaluate.py:302-324 (ensemble): per point normalise both feature sources
 * (x / (|x| + 1e-5)), take the source whose best fp16 score is larger (fusion wins
 * only if strictly larger), re-score the selected UN-normalised fp16 features.
 * Each source has its own (nullable) gather: the reference gathers the distilled
 * voxel features with inds_reverse while the fused features are already per point.
 * sel (nullable) uint8 [n] = 1 where the fusion feature was selected.            */
/* labels[p] = argmax over the first c columns of row (gather ? gather[p] : p) of a float32 score matrix with row stride ld
 * (the first NaN wins, otherwise the first maximum): `torch.max(pred, 1)[1]` of run/evaluate.py:292 fused with the point -> voxel gather `[inds_reverse]`,
 * for scores that exist per VOXEL (the fused-head query).  Indices outside [0, n_rows) read row 0.  */
int osn_rows_argmax(const float* scores, int64_t ld, int c, const int64_t* gather, int64_t n_pts, int64_t n_rows,
                    int64_t* labels, osn_stream_t stream);
size_t osn_query_ensemble_ws_bytes(int64_t n);
int osn_query_ensemble(const float* X_distill, const int64_t* gather_distill,
                       const float* X_fusion, const int64_t* gather_fusion,
                       const void* text_f16, void* scores_f16, int64_t* argmax, uint8_t* sel,
                       int64_t n, int d, int c, void* ws, size_t ws_bytes, osn_stream_t stream);
/* Test-repeat votes (run/evaluate.py:390,397,416: `preds.append(pred.cpu())`, `torch.cat`, `store = pred + store` on
 * CPU fp16 tensors).  The same queries with a vote epilogue: instead of storing the fp16 score of (point p, label l) the
 * kernel adds it to the caller-owned fp16 matrix,
 *     votes_f16[p * c + l] = fp16_rne(float(votes_f16[p * c + l]) + float(score_f16))
 * which is torch's CPU half add (computed in fp32, rounded once).  Each cell has one owner: no atomics, deterministic.
 * votes_f16 is [n, c], already offset to the scene's first row; 16-byte aligned when c % 8 == 0, else 2-byte aligned.
 * No score matrix is written; argmax (nullable) is the per-scene label of this repeat's scores, as above.            */
int osn_cosine_query_vote(const float* X, const int64_t* gather, const void* text_f16,
                          void* votes_f16, int64_t* argmax, int64_t n, int d, int c,
                          osn_stream_t stream);
int osn_query_ensemble_vote(const float* X_distill, const int64_t* gather_distill,
                            const float* X_fusion, const int64_t* gather_fusion,
                            const void* text_f16, void* votes_f16, int64_t* argmax, uint8_t* sel,
                            int64_t n, int d, int c, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- open-vocabulary evaluation (csrc/evaluate.hip) ------------------------------------------------------------ *
 * Replaces run/evaluate.py:397-424 (`store.float().max(1)[1]`, `mapper[...]`, `[~mask] = 256`) and util/metric.py:9-25
 * (confusion_matrix).  One pass over n points; exactly one prediction source:
 *   votes_f16  fp16 [n, c_in] (1 <= c_in <= 256): pred = Tensor.max(1)[1] on CPU (first NaN wins, else the lowest column
 *              among equal maxima), or
 *   ids        int64 [n]: given predictions (the one-repeat path, run/evaluate.py:387; 256 = no feature).
 * mapper (nullable) int64 [n_map]: pred = mapper[pred] (nuScenes 43 -> 16); has_feature (nullable) uint8 [n]: 0 -> 256.
 * labels int64 [n]: 255 is ignored.  confusion int64 [(c_out + 1) * c_out], [pred, gt], ACCUMULATED: rows 0 .. c_out-1 are
 * metric.confusion_matrix, row c_out counts the no-feature points per gt class.  1 <= c_out <= 254.
 * err int32 [1] (device) is ORed with: 1 a prediction outside the mapper, 2 a gt outside [0, c_out) that is not 255,
 * 4 a counted prediction outside [0, c_out) that is not 256; osn_eval_check synchronises and turns it into OSN_E_ARG.
 * hist: -1 chooses (LDS up to 90 classes), 1 counts in an LDS histogram per workgroup (c_out <= 160), 0 uses int64
 * atomics on the matrix.                                                                                         */
int osn_eval_confusion(const void* votes_f16, const int64_t* ids, int64_t n, int c_in, const int64_t* labels,
                       const int64_t* mapper, int64_t n_map, const uint8_t* has_feature, int c_out,
                       int64_t* confusion, int32_t* err, int hist, osn_stream_t stream);
int osn_eval_check(const int32_t* err, osn_stream_t stream);

/* ---- text search over a bank of scenes (csrc/search.hip) -------------------------------------------------------- *
 * The second half of the open-vocabulary query (README "Applications": scene exploration, rare object search in a 3D
 * scene database): heat-maps for arbitrary queries and the k best points of every scene, over a bank of per-point fp16
 * features -- the rows run/evaluate.py:232-235,328-330 saves as <scene>_openscene_feat_<feature_type>.npy.
 *
 * The append: bank_f16[row0 + i, :] = fp16_rne(X[gather ? gather[i] : i, :]) for i < n -- X[inds_reverse].half() of
 * run/evaluate.py:290 without the float32 [n, d] intermediate.  X float32 [n_rows, d]; gather (nullable) int64 [n];
 * d % 8 == 0.  A gather entry outside [0, n_rows) reads and writes nothing for that row and ORs bit 1 into the device
 * word err (int32 [1]).
 * The check synchronises and turns the bits of err into OSN_E_ARG: 1 a bad gather index, 2 scene offsets that do
 * not start at 0, ascend and end within the bank, 4 a scene longer than max_scene_rows (8, 16, 32: the
 * pool's, below.)
 *
 * The search: bank fp16 [n, d]; scene_offsets int64 [n_scenes + 1] (device), ascending from 0, empty scenes allowed;
 *   max_scene_rows >= the longest scene (sizes the grid); queries fp16 [q, d], L2-normalised by the caller
 *   (util/util.py:41-44); 1 <= q <= 1024; 1 <= k <= 128; thresholds (nullable) float32 [q].
 *   score(p, j) with h = the stored fp16 row p, hf = h.float():
 *     normalize = 1   run/evaluate.py:305,310  (hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half() @ t.t()
 *     normalize = 0   run/evaluate.py:291      h @ t.t()
 *   fp16 MFMA, fp32 accumulate, one rounding to fp16; with normalize the fp32 accumulator is divided by (norm + 1e-5),
 *   the norm taken from the same chunks that feed the MFMA (the bank is read once) -- within 2^-11 of rounding the
 *   normalised vector first, for unit-norm queries.
 *   The arithmetic contract (tests/search_bounds.py, held on the device by tests/test_gpu_search_bounds.py): with v the
 *   stored row, S = sum v_k t_k, A = sum |v_k| |t_k|, N = sqrt(sum v_k^2) in float64, c = 2e-6 (the bound of every fp32-
 *   accumulating MFMA contraction here) and DELTA = 1.4e-5 (four times the measured error of fp32 sqrtf(sum v^2) + 1e-5f),
 *     normalize = 0   fp16_rne(S - c A) <= score <= fp16_rne(S + c A)
 *     normalize = 1   fp16_rne(L) <= score <= fp16_rne(U), L and U the least and the largest of
 *                     (S -+ c A) / ((N + 1e-5) (1 -+ DELTA)) over the four sign choices
 *   each end rounded from float64 in one step (a raw score beyond the fp16 range is +-inf).  fp16 subnormals of rows and
 *   queries count in full.  A row of zeros (of either sign) scores +0.0 bit for bit; a row that holds a NaN scores NaN for
 *   every query; a row that holds an inf scores NaN for every query with normalize = 1 and S itself with normalize = 0.
 *   heat (nullable) fp16 [n, q]; topk_scores fp16 [n_scenes, q, k]; topk_points int64 [n_scenes, q, k] = the row inside
 *   its scene, ordered by higher score, then lower row; NaN orders below every number (and is stored as NaN in heat);
 *   a scene with fewer than k points pads with (-inf, -1).  counts (nullable, needs thresholds) int64 [n_scenes, q] =
 *   the scene's points with score >= thresholds[j].  n_scenes = 0 writes the heat-map only.  Integer atomics only:
 *   bitwise repeatable.  Offsets are clamped before use (nothing is read out of bounds) and reported through err. */
int osn_bank_append(const float* X, int64_t n_rows, const int64_t* gather, int64_t n, int d, void* bank_f16,
                    int64_t row0, int32_t* err, osn_stream_t stream);
int osn_bank_check(const int32_t* err, osn_stream_t stream);
size_t osn_bank_search_ws_bytes(int64_t n, int n_scenes, int q, int k, int64_t max_scene_rows);
int osn_bank_search(const void* bank_f16, int64_t n, int d, const int64_t* scene_offsets, int n_scenes,
                    int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                    const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                    int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);

/* The same bank at one byte per element: a row x (X[inds_reverse] of run/evaluate.py:290, float32, or float16 widened
 * exactly) is stored as d OCP e4m3fn codes and one exponent byte e; its stored value is v_i = float(code_i) * 2^e.
 *   amax = max |x_i|.  A non-finite element: e = 0 and every code of the row is an e4m3 NaN (code & 0x7F == 0x7F).
 *   amax == 0: e = 0.  Otherwise e = the smallest integer >= -120 with amax * 2^-e <= 448 (-120 <= e <= 120).
 *   code_i = e4m3fn(x_i * 2^-e): the scaling is exact in float32, the conversion one round-to-nearest-even that keeps
 *   the sign of zero and never saturates.
 * osn_bank_append_fp8: X float32 (x_is_f16 = 0) or float16 (1) [n_rows, d]; d % 16 == 0; codes uint8 [.., d] and exps
 *   int8 [..] receive rows row0 .. row0 + n; gather and err as osn_bank_append.  One wave per row; rows up to 2048 wide
 *   are read once, wider rows read their tail twice.
 * osn_bank_search_fp8: osn_bank_search over (codes, exps) -- the remaining arguments, the workspace
 *   (osn_bank_search_ws_bytes), selection, padding, counts, NaN order and repeatability are osn_bank_search's.  With c the
 *   row of code values, t an fp16 query and acc = sum c_i t_i (fp16 MFMA, exact widening of the codes, fp32 accumulate):
 *     normalize = 1   run/evaluate.py:305,310  acc / (sqrt(sum c_i^2) + 1e-5 / 2^e), rounded to fp16 once
 *     normalize = 0   run/evaluate.py:291      acc * 2^e, rounded to fp16 once
 *   The first is acc * 2^e / (sqrt(sum c_i^2) * 2^e + 1e-5) with 2^e divided out (1e-5 / 2^e is exact in fp32): the same
 *   bits wherever that form stays inside fp32, and a cosine in [-1, 1] at every exponent up to e = 120, where the scaled
 *   norm passes 2^128 (from e = 115 on at d = 768) and the scaled form gave 0 or NaN for a finite row.
 *   A zero row scores exactly +0.0, a NaN row (a row that held a NaN or an inf) NaN for every query.  The contract of
 *   osn_bank_search holds with v_i = code_i * 2^e: same c, same DELTA, every exponent byte.                          */
int osn_bank_append_fp8(const void* X, int x_is_f16, int64_t n_rows, const int64_t* gather, int64_t n, int d,
                        uint8_t* codes, int8_t* exps, int64_t row0, int32_t* err, osn_stream_t stream);
int osn_bank_search_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* scene_offsets,
                        int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                        const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                        int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);

/* Search with negative queries: the heat-map holds relevancies against the best of m negative phrases ("object", "things",
 * "stuff", "texture" in the LERF line of work) in place of raw cosines, so that one threshold means the same for every
 * query.  Inputs beyond osn_bank_search's / osn_bank_search_fp8's: negatives fp16 [m, d], L2-normalised by the caller,
 * 16-byte aligned, 1 <= m <= 1024; temperature float32, finite and > 0.  With s(p, j) the fp16 score osn_bank_search writes
 * for query j and g(p, i) the one it writes for negative i as a query (either normalize mode; bit for bit, whichever
 * column group a column falls in):
 *     nmax(p)   = max_i float(g(p, i))                          a NaN among them makes nmax NaN
 *     z(p, j)   = (float(s(p, j)) - nmax(p)) / temperature      fp32, IEEE, as written
 *     rel(p, j) = fp16_rne(1.0f / (1.0f + expf(-z)))
 * = min_i softmax([s, g_i] / temperature)[0], the pairwise-softmax relevancy (the sigmoid is monotone).  NaN in gives NaN
 * out (inf - inf included); saturation to exactly 0 or 1 is expected and leaves large tie groups to the selection's total
 * order.  heat fp16 [n, q] holds rel; the negatives get no column in heat or in the workspace, which stays
 * osn_bank_search_ws_bytes(n, n_scenes, q, ...).  topk_*, thresholds and counts act on rel; padding, NaN order, clamped
 * offsets, the err bits, integer atomics only and bitwise repeatability are osn_bank_search's.  One pass over the bank:
 * the negatives' column groups run first through the same MFMA loop and leave only a per-row maximum in LDS.          */
int osn_bank_search_contrast(const void* bank_f16, int64_t n, int d, const int64_t* scene_offsets, int n_scenes,
                             int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                             const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                             int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                             const void* negatives_f16, int m, float temperature);
int osn_bank_search_contrast_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* scene_offsets,
                                 int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                                 const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                                 int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                                 const void* negatives_f16, int m, float temperature);

/* Two banks searched as one: the 2D-3D ensemble of run/evaluate.py:302-324 at query time.  A = bank_f16 / (codes, exps), in
 * the reference the distilled features; B = other_f16 / (other_codes, other_exps), the fused ones: the same kind, n and d,
 * row p of both the same point.  The choice of a source depends on the text rows (mask_ of :319 is a function of
 * text_features), so it is made here, in the pass that reads the two banks, and not stored.
 *   s_X(p, j)   the fp16 score osn_bank_search[_fp8] writes for row p of bank X and query j under the caller's normalize
 *   n_X(p, j)   the same with normalize = 1
 *   r_X(p, j)   with negatives, the relevancy osn_bank_search_contrast[_fp8] writes for bank X
 * all three pure functions of one stored row and the query rows, formed here by the same code, bit for bit.
 *   x_X = s_X, or r_X with negatives (m >= 1; m = 0 with null negatives_f16 means plain scores).
 * mode 0, "vocabulary" (:318-321):  source(p) = max_j n_A(p, j) < max_j n_B(p, j).  The maximum propagates NaN; the
 *   comparison is IEEE, so equal values, -0 against +0 and a NaN on either side give 0 (A).  The pick is always taken on the
 *   normalised scores, whatever normalize is; negatives take no part in it.  Row p of heat is x_B(p, :) where source(p), else
 *   x_A(p, :): a query's column depends on the other queries of the call.  source uint8 [n], required.
 * mode 1, "query" (the commented variant, :312-316):  source(p, j) = x_A(p, j) < x_B(p, j), IEEE;  heat(p, j) = x_B(p, j)
 *   where source(p, j), else x_A(p, j): column j depends on query j alone.  source uint8 [n, q] row-major, nullable.
 * Everything after the heat-map -- heatT, topk_*, thresholds, counts, padding, NaN order, err bits, repeatability, the workspace
 * osn_bank_search_ws_bytes(n, n_scenes, q, ...) -- is osn_bank_search's, on that heat-map.  q, m <= 1024, k <= 128.
 * One launch, 128 rows per workgroup.  Vocabulary: the queries' column groups over A's rows, then over B's, keeping only each
 * row's maximum; the pick; then the walk of the plain (or contrast) search, every row fetched from its chosen source.  Query:
 * every column group over A, then over B, A's fp16 values held in registers.  Each bank comes from HBM once; the further
 * walks read the workgroup's rows from cache.                                                                             */
int osn_bank_search_ensemble(const void* bank_f16, const void* other_f16, int64_t n, int d, const int64_t* scene_offsets,
                             int n_scenes, int64_t max_scene_rows, const void* queries_f16, int q, int normalize, int k,
                             const float* thresholds, void* heat_f16, void* topk_scores_f16, int64_t* topk_points,
                             int64_t* counts, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream,
                             const void* negatives_f16, int m, float temperature, int mode, uint8_t* source);
int osn_bank_search_ensemble_fp8(const uint8_t* codes, const int8_t* exps, const uint8_t* other_codes, const int8_t* other_exps,
                                 int64_t n, int d, const int64_t* scene_offsets, int n_scenes, int64_t max_scene_rows,
                                 const void* queries_f16, int q, int normalize, int k, const float* thresholds, void* heat_f16,
                                 void* topk_scores_f16, int64_t* topk_points, int64_t* counts, int32_t* err, void* ws,
                                 size_t ws_bytes, osn_stream_t stream, const void* negatives_f16, int m, float temperature,
                                 int mode, uint8_t* source);

/* ---- descriptors of point sets over the bank (csrc/pool.hip) ----------------------------------------------------- *
 * The way back from points to a feature vector (README "Applications": "retrieve examples based on similarities", room
 * type, labelling a found object): the sum of the normalised stored rows of every group of a list of bank rows; the mean
 * of a group is its descriptor.  bank / (codes, exps), n, d: the bank of osn_bank_search / osn_bank_search_fp8,
 * d <= OSN_BANK_POOL_MAX_DIM.  Groups in CSR form: starts int64 [n_groups + 1] (device), ascending, starts[0] = 0,
 * starts[n_groups] = n_entries; rows (nullable) int64 [n_entries] = bank rows, null: entry i is bank row i (whole scenes:
 * starts = the bank's scene offsets); weights (nullable) float32 [n_entries], null: 1.  With v the stored row of an entry
 * (the fp16 values, or float(code) * 2^e, decoded exactly) and w its weight, the entry's term is
 *     normalize = 1   run/evaluate.py:305   w * v / (v.norm() + 1e-5)     the norm in fp32 over the stored values
 *     normalize = 0                         w * v
 * sum float32 [n_groups, d] = the terms of a group added in fp32; wsum float32 [n_groups] = its weights; count int64
 * [n_groups] = its entries.  Entry order is accumulation order, duplicate rows are allowed, an empty group gives zeros, a
 * NaN row makes its own group NaN and no other.
 * Determinism: no floating-point atomics.  A group is cut into chunks of OSN_BANK_POOL_CHUNK consecutive entries; a
 * chunk is reduced in a fixed order (wave w of four takes entries w, w + 4, ..., the waves are added in wave order) into an
 * fp32 partial in ws, a second launch adds a group's partials in ascending chunk order.  The result is a function of
 * the input arrays alone -- bitwise repeatable -- and a group's bits do not depend on its place in the list.
 * An entry whose row is outside [0, n) or whose weight is negative or not finite is skipped (its row loads are made from
 * a clamped address inside the bank and not used; it enters neither sum, wsum nor count) and ORs 8 (row) or 16 (weight)
 * into the bank's err word; starts that do not ascend from 0 to n_entries are clamped before use and OR 32;
 * osn_bank_check turns the bits into OSN_E_ARG.
 * ws: osn_bank_pool_ws_bytes(n_groups, n_entries, d) bytes.  Asynchronous.                                           */
#define OSN_BANK_POOL_CHUNK 512
#define OSN_BANK_POOL_MAX_DIM 1024
size_t osn_bank_pool_ws_bytes(int64_t n_groups, int64_t n_entries, int d);
int osn_bank_pool(const void* bank_f16, int64_t n, int d, const int64_t* starts, int64_t n_groups, const int64_t* rows,
                  int64_t n_entries, const float* weights, int normalize, float* sum, float* wsum, int64_t* count,
                  int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);
int osn_bank_pool_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* starts, int64_t n_groups,
                      const int64_t* rows, int64_t n_entries, const float* weights, int normalize, float* sum, float* wsum,
                      int64_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- second moments of point sets over the bank (csrc/gram.hip) -------------------------------------------------- *
 * How the features of a point set are spread: the Gram matrix X^T X of its rows -- covariance, principal directions and
 * explained variance follow on the host (openscene_amd.pca) -- next to the first moment from the same operands.  bank /
 * (codes, exps), n, d, the CSR groups (starts, n_groups, rows nullable, n_entries), err and the guards are exactly
 * osn_bank_pool's; there are no weights.  With v the stored row of an entry (the fp16 values, or float(code) * 2^e,
 * decoded exactly):
 *     normalize = 1:  h = fp16_rne(v / (||v|| + 1e-5)), the norm in fp32 over the stored values -- run/evaluate.py:305,310
 *                     including its .half(); the quotient is formed as v * r with r = fp32(2^e / (||c|| * 2^e + 1e-5)),
 *                     within an fp32 ulp of it
 *     normalize = 0:  h = fp16_rne(v): exact for an fp16 bank, and for fp8 rows whose values lie in fp16's range
 *     gram  float32 [n_groups, d, d]:  gram[g, a, b] = sum over the entries of group g of h_a * h_b
 *     sum   float32 [n_groups, d]:     sum[g, a]     = sum over the entries of group g of h_a   (the same h)
 *     count int64   [n_groups]:        the entries of the group that were not skipped
 * The Gram matrix is taken with fp16 MFMA: a product of two fp16 values is exact in the fp32 accumulator, only the
 * accumulation rounds.  Only the 128-column tiles on or above the diagonal are computed; the launch that adds the
 * partials writes an element and its mirror image from the same value: gram[g] is bitwise symmetric.
 * Determinism: no floating-point atomics.  A group is cut into slices of OSN_BANK_GRAM_SLICE consecutive entries, counted
 * from the group's own start; a slice x tile pair is one fp32 partial in ws; a second launch adds a group's partials in
 * ascending slice order.  The result is a function of the input arrays alone -- bitwise repeatable -- and a group's bits
 * do not depend on its place in the list.
 * Guards: an entry whose row is outside [0, n) is skipped (its loads are made from a clamped address inside the bank and not
 * used; it enters neither gram, sum nor count) and ORs 8 into the bank's err word; starts that do not ascend from 0 to n_entries are clamped before use and OR 32;
 * osn_bank_check turns the bits into OSN_E_ARG.  An empty group gives zeros; a NaN row makes its own group NaN and no other.
 * ws: osn_bank_gram_ws_bytes(n_groups, n_entries, d) bytes -- 64 KiB per slice and tile pair.  Asynchronous.            */
#define OSN_BANK_GRAM_SLICE 2048
size_t osn_bank_gram_ws_bytes(int64_t n_groups, int64_t n_entries, int d);
int osn_bank_gram(const void* bank_f16, int64_t n, int d, const int64_t* starts, int64_t n_groups, const int64_t* rows,
                  int64_t n_entries, int normalize, float* gram, float* sum, int64_t* count, int32_t* err, void* ws,
                  size_t ws_bytes, osn_stream_t stream);
int osn_bank_gram_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* starts, int64_t n_groups,
                      const int64_t* rows, int64_t n_entries, int normalize, float* gram, float* sum, int64_t* count,
                      int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- bank rows matched to exemplars (csrc/match.hip) ------------------------------------------------------------- *
 * For each of n_rows bank rows the k most similar of n_exemplars exemplar rows -- label by example, correspondences,
 * novelty -- without an n_rows x n_exemplars array anywhere.  bank / (codes, exps), n, d, err and the row guard are
 * osn_bank_gram's; `rows` int64 [n_rows] (device) or null: entry i is bank row i.
 *   operand  u = fp16_rne(v * r) with v the stored row (the fp16 values, or float(code) * 2^e decoded exactly) and r the fp32
 *            factor 1 / (||v|| + 1e-5) (run/evaluate.py:305,310; fp8: 2^e / (||c|| * 2^e + 1e-5)); normalize = 0: u = fp16_rne(v).
 *            Bit for bit the operand h of osn_bank_gram.
 *   score    s(p, e) = the fp32 MFMA accumulation (v_mfma_f32_16x16x32_f16) of the exact fp16 x fp16 products over d in
 *            ascending steps of 32 from a zero accumulator, zeros past d: a function of the two operand rows and d alone, not
 *            of n_rows, n_exemplars, the position of either row, k, or how the exemplars are split over workgroups.
 *   order    one 64-bit key per candidate: the monotone 32-bit image of the score in the high word, 0xFFFFFFFF - position in
 *            the low word; the largest key is the best.  A NaN ranks below -inf; -0 ranks as, and is returned as, +0; equal
 *            scores go to the lower exemplar position.
 *   result   idx int32 [n_rows, k]: positions in the exemplar list, -1 past count; score float32 [n_rows, k], -inf past
 *            count; count int32 [n_rows] = min(k, n_exemplars); a row's list in descending key order.  No floating-point
 *            atomics: bitwise repeatable.
 * osn_bank_unit_rows gathers a row list and writes its operands as the fp16 image [n_rows, d] (16-byte aligned) that
 * osn_bank_match takes as `exemplars_f16`; the query side is read straight from the bank and its operands are formed in
 * the kernel.  A row outside [0, n) writes zeros (unit_rows) or is matched as a zero row (match) and ORs 8 into the err
 * word; osn_bank_check turns the bit into OSN_E_ARG.
 * Limits: d % 8 == 0 (fp16 bank) or d % 16 == 0 (fp8 bank), d <= OSN_BANK_POOL_MAX_DIM, 1 <= k <= OSN_BANK_MATCH_MAX_K,
 * 1 <= n_exemplars < 2^31; n_rows = 0 returns at once.  A workgroup owns OSN_BANK_MATCH_TILE_Q query rows and a contiguous
 * range of tiles of OSN_BANK_MATCH_TILE_E exemplars; the tiles are cut into `splits` ranges (0: chosen here so that the grid
 * fills the device; at most OSN_BANK_MATCH_MAX_SPLITS) whose k keys per row a second launch merges.  The result does not
 * depend on `splits`.
 * ws: osn_bank_match_ws_bytes(n_rows, n_exemplars, d, k, splits) = 8 * n_rows * k * splits bytes (the splits in effect) plus a
 * constant below 8 KiB: it never grows with n_rows * n_exemplars.  Asynchronous.                                        */
#define OSN_BANK_MATCH_MAX_K 8
#define OSN_BANK_MATCH_TILE_Q 64
#define OSN_BANK_MATCH_TILE_E 256
#define OSN_BANK_MATCH_MAX_SPLITS 64
int osn_bank_unit_rows(const void* bank_f16, int64_t n, int d, const int64_t* rows, int64_t n_rows, int normalize,
                       void* out_f16, int32_t* err, osn_stream_t stream);
int osn_bank_unit_rows_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* rows, int64_t n_rows,
                           int normalize, void* out_f16, int32_t* err, osn_stream_t stream);
size_t osn_bank_match_ws_bytes(int64_t n_rows, int64_t n_exemplars, int d, int k, int splits);
int osn_bank_match(const void* bank_f16, int64_t n, int d, const int64_t* rows, int64_t n_rows, int normalize,
                   const void* exemplars_f16, int64_t n_exemplars, int k, int splits, int32_t* idx, float* score,
                   int32_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);
int osn_bank_match_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* rows, int64_t n_rows,
                       int normalize, const void* exemplars_f16, int64_t n_exemplars, int k, int splits, int32_t* idx,
                       float* score, int32_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- objects in heat-maps (csrc/objects.hip) -------------------------------------------------------------------- *
 * What the README "Applications" do with a heat-map -- rare object search in a 3D scene database, image-based 3-D object
 * detection, interactive object search -- needs objects, not points: WHERE the matches are, how many, how large, how
 * confident.  An object of query j is a connected component (26- or 6-neighbourhood of the 3^3 self-map) of the voxels
 * that hold at least one HIT: a point with a finite score and float(heat[p, j]) >= thresholds[j].
 *
 * Inputs shared by the two calls: heat fp16 [n, q] (osn_bank_search's); thresholds float32 [q]; inverse int32 [n] =
 *   the voxel row of every point; coords4 int32 [n_voxels, 4] = (scene, x, y, z) rows in the order the self-map was built
 *   from (osn_coords_unique); scene_offsets int64 [n_scenes + 1], ascending from 0 to n; n < 2^22, q <= 1024,
 *   q * n_voxels < 2^31.  ws: osn_objects_ws_bytes(n_voxels, n_scenes, q) bytes -- two words per (query, voxel) and two per
 *   (scene, query); it carries the labels from the first call to the second.
 *
 * osn_objects_label (interactive object search: one call labels every query): marks the active (query, voxel) pairs,
 *   unites them over nbr int32 [27, n_voxels] (osn_kmap_build_self, ksize 3; the 13 offsets below the centre, or the 3
 *   face offsets among them for connectivity 6) with a lock-free union-find -- larger root under smaller, compare-and-
 *   swap, path halving; the partition does not depend on scheduling -- flattens, and numbers the components of every
 *   (scene, query).  Zeroes and uses the device word err (int32 [1]); SYNCHRONISES once to return the number of components
 *   to the host (*n_components_host) together with err: bad offsets, an inverse / batch / neighbour entry out of range
 *   (such entries are skipped, never dereferenced) -> OSN_E_ARG.
 *
 * osn_objects_find (rare object search / 3-D detection: ranked objects per scene): records = a buffer of
 *   osn_objects_records_bytes(n_components) bytes (scratch grows with the components, not with q * n_voxels * record).
 *   Per component, with integer atomics only (bitwise repeatable): n_points, n_voxels, score_sum = sum of score * 2^24
 *   (exact: every finite fp16 is a multiple of 2^-24), the peak as a packed (score key, ~point) 64-bit max -- the lowest
 *   row inside the scene among the maxima --, vox_sum int64 [3], and the float32 box of the members' xyz [n, 3] through
 *   order-preserving integer min / max.  combine = 1 merges the lanes of a wave that target one record before the
 *   atomic (0: every hit issues its own; for measurements).  Per (scene, query): objects with n_points < min_points are
 *   dropped, the rest ordered by peak score descending, then peak point ascending; the first max_objects (1 .. 64) are
 *   written to out_* [n_scenes, q, max_objects] (vox_sum / box_*: [.., 3]); out_n_objects int64 [n_scenes, q] counts the
 *   objects that passed the filter; padding = (n_points 0, peak_point -1, peak_score -inf, zeros).  point_object
 *   (nullable) int32 [n, q] = the rank of the kept object a hit belongs to, else -1.  Asynchronous. */
size_t osn_objects_ws_bytes(int64_t n_voxels, int n_scenes, int q);
size_t osn_objects_records_bytes(int64_t n_components);
int osn_objects_label(const void* heat_f16, int64_t n, int q, const float* thresholds, const int32_t* inverse,
                      const int32_t* coords4, int64_t n_voxels, const int32_t* nbr, int connectivity,
                      const int64_t* scene_offsets, int n_scenes, int32_t* err, void* ws, size_t ws_bytes,
                      int64_t* n_components_host, osn_stream_t stream);
int osn_objects_find(const void* heat_f16, const float* xyz, int64_t n, int q, const float* thresholds,
                     const int32_t* inverse, const int32_t* coords4, int64_t n_voxels, const int64_t* scene_offsets,
                     int n_scenes, int64_t n_components, int min_points, int max_objects, int combine,
                     int64_t* out_n_points, int64_t* out_n_voxels, void* out_peak_score_f16, int64_t* out_peak_point,
                     int64_t* out_score_sum, int64_t* out_vox_sum, float* out_box_min, float* out_box_max,
                     int64_t* out_n_objects, int32_t* point_object, const void* ws, size_t ws_bytes, void* records,
                     size_t records_bytes, osn_stream_t stream);

/* ---- regions without a prompt (csrc/regions.hip) ---------------------------------------------------------------- *
 * README "Applications": "open-vocabulary 3D scene understanding and exploration" -- materials, affordances, room type,
 * "what is in this room?" -- needs a partition of a scene that exists before anyone has typed a word and serves every
 * later prompt.  A region is a connected component of the graph over the voxels whose edges are the pairs of neighbouring
 * voxels (3^3 self-map; 26 or 6 neighbours) with agreeing features: single linkage.  All three calls OR their error bits
 * into the device word err (int32 [1], zeroed by the caller): 1 = a neighbour row outside [-1, n_voxels), 2 = a point's
 * voxel row outside [0, n_voxels), 4 = a region entry outside [-1, n_regions).  Such entries are skipped, never
 * dereferenced.  All three are asynchronous and need no workspace.
 *
 * osn_regions_edges (the hot path): vox fp16 [n_voxels, d] (device, 16-byte aligned), d % 8 == 0, 8 <= d <=
 *   OSN_BANK_POOL_MAX_DIM; nbr int32 [27, n_voxels] (osn_kmap_build_self, ksize 3); connectivity 26 or 6.
 *   sim float32 [n_off, n_voxels]: n_off = 13 for connectivity 26 -- the offsets below the centre, k = 0 .. 12 -- and 3 for
 *   connectivity 6 -- k = 4, 10, 12 (-z, -y, -x), in that order.  With u = nbr[k_i, v]:
 *       sim[i, v] = sum over c of float(vox[v, c]) * float(vox[u, c]),  accumulated in fp32
 *   No division: the caller supplies unit rows.  An absent neighbour (u < 0) gives -inf; u >= n_voxels gives -inf and ORs
 *   bit 1; a NaN anywhere in either row gives NaN.  The self-map is its own mirror, so every undirected edge is computed
 *   once.  A product of two fp16 values is exact in fp32, so only the additions round; their order is fixed (a lane adds
 *   the products of its 16-byte vectors in element order, the lanes of the wave are added by an xor butterfly): no
 *   floating-point atomics, two calls give the same bits.  fp16 subnormals enter with their value.
 *
 * osn_regions_label: voxels v and u = nbr[k_i, v] are united iff u is a valid row and sim[i, v] >= threshold (a float32
 *   comparison; threshold finite; NaN and -inf never unite), with the union-find of osn_objects_label: larger root under
 *   smaller, compare-and-swap, path halving, a flatten launch after the unite launch.  voxel_root int32 [n_voxels]:
 *   the smallest voxel row of v's component -- a canonical labelling that does not depend on scheduling.  Every voxel
 *   belongs to exactly one component; a voxel without an accepted edge is its own.
 *
 * osn_regions_records: voxel_region int32 [n_voxels] with values in -1 .. n_regions - 1 (-1: in no region); xyz float32
 *   [n, 3], inverse int32 [n] (point -> voxel row), coords4 int32 [n_voxels, 4] (scene, x, y, z; 16-byte aligned).  Per
 *   region, with integer atomics only (exact, bitwise repeatable): n_points int64, n_voxels int64, vox_sum int64 [.., 3]
 *   = the sum over the region's POINTS of their voxel's (x, y, z) (as in osn_objects_find), box_min / box_max float32
 *   [.., 3] over the points' xyz through order-preserving integer min / max (a region without points: zeros), scene
 *   int32 = the scene column of the region's smallest voxel row (-1: a region without voxels).  Points whose voxel has
 *   region -1 are counted nowhere.                                                                                   */
int osn_regions_edges(const void* vox_f16, int64_t n_voxels, int d, const int32_t* nbr, int connectivity, float* sim,
                      int32_t* err, osn_stream_t stream);
int osn_regions_label(const float* sim, const int32_t* nbr, int64_t n_voxels, int connectivity, float threshold,
                      int32_t* voxel_root, int32_t* err, osn_stream_t stream);
int osn_regions_records(const int32_t* voxel_region, int64_t n_voxels, int64_t n_regions, const float* xyz,
                        const int32_t* inverse, int64_t n, const int32_t* coords4, int64_t* n_points,
                        int64_t* n_voxels_out, int64_t* vox_sum, float* box_min, float* box_max, int32_t* scene,
                        int32_t* err, osn_stream_t stream);

/* ---- merge regions by mean feature: region adjacency and star contraction (csrc/merge.hip) ----------------------- *
 * Single linkage joins the two ends of a chain of pairwise similar voxels however different they are.  The second stage
 * over-segments with a strict threshold and then merges ADJACENT regions whose mean features agree; the mean of a grown
 * region does not drift along a chain.  The loop is openscene_amd/merge.py; these are the kernels of one round.  All
 * calls OR their error bits into the regions err word (above: 1, 2, 4) and add 8 = a pair end outside [0, n_regions).
 * Bad entries are skipped, never dereferenced.  All are asynchronous; only osn_merge_round needs a workspace.
 *
 * Contacts.  voxel_region int32 [n_voxels] with values in -1 .. n_regions - 1, nbr int32 [27, n_voxels].  A contact is a
 *   voxel pair (v, u = nbr[k_i, v]) over the offsets below the centre (13, or the 3 faces k = 4, 10, 12 for connectivity
 *   6, as in osn_regions_edges) with u a valid row and both regions >= 0 and different.  Voxels of region -1 touch
 *   nothing; scenes never touch, because the table holds no such neighbours.  The adjacency list is the sorted distinct
 *   pairs (lo < hi) with their contact counts.
 * osn_merge_contacts: key int64 [n_off, n_voxels] = lo << 32 | hi of the contact of (i, v), or -1 where there is none.
 *   u >= n_voxels ORs bit 1, a region entry outside [-1, n_regions) bit 4; both give -1.  Compaction, sorting and
 *   counting the distinct keys are the caller's (torch.unique).
 *
 * Region rows.  S float32 [R, d] starts as the pool kernel's sums of the regions (osn_bank_pool*, either bank kind); the
 *   unit rows of a round are X = where(n > 0, S / n, 0) rounded to fp16, n = ||S|| per row, formed by the caller.
 * osn_rows_pair_dot (the hot path): rows fp16 [n_rows, d] (16-byte aligned), d % 8 == 0, 8 <= d <= OSN_BANK_POOL_MAX_DIM;
 *   lo, hi int32 [n_pairs]; n_pairs < 2^32 - 1.
 *       sim[e] = sum over c of float(rows[lo[e], c]) * float(rows[hi[e], c]),  accumulated in fp32
 *   with the lane layout and the order of additions of osn_regions_edges (one shared body, csrc/rowdot.h: a lane adds the
 *   products of its 16-byte vectors in element order, then an xor butterfly over the lanes): for the same two rows the
 *   two entries give the same bits, whichever is lo.  An end outside [0, n_rows) gives -inf and ORs bit 8; a NaN in
 *   either row gives NaN.  A wave takes a fixed run of consecutive pairs, so a row with thousands of partners costs no
 *   more per pair than any other.  No LDS, no floating-point atomics: two calls give the same bits.
 *
 * A round.  The caller lists the pairs with contacts >= min_contact in ascending (lo, hi) order; e is the index.  An
 *   edge is eligible iff sim[e] >= threshold (a float32 comparison; threshold finite; NaN and -inf never pass); a pair
 *   with lo == hi is ignored.  Its key is (order-preserving uint32 of sim[e]) << 32 | (0xFFFFFFFF - e), the same from
 *   both ends: greater similarity wins, then the lower edge index; -0 orders below +0.  best[a] is the greatest key
 *   among a's eligible edges (a 64-bit integer atomic maximum: independent of scheduling).  An edge is mutual when both
 *   ends name it as their best.  Region a with best edge (a, b) is united with b iff that edge is mutual or b's best
 *   edge is mutual -- a mutual pair plus the regions that point at it, a star.  The globally greatest eligible key is
 *   always mutual, so a round with an eligible edge merges something.
 * osn_merge_round: lo, hi int32 [n_pairs], sim float32 [n_pairs], n_pairs < 2^32 - 1, n_regions < 2^31 (both checked
 *   on the host); ws: osn_merge_ws_bytes(n_regions) bytes, 8-byte aligned (one 64-bit word per region).  parent int32
 *   [n_regions]: every region's smallest group member, flattened (the union-find of osn_regions_label).  Numbering
 *   the groups in ascending order of parent keeps the canonical numbering, ascending smallest voxel row.  Four
 *   launches: preset, best, unite, flatten.  An end out of range ORs bit 8 and the pair is skipped.
 *
 * osn_rows_fold: src float32 [n_src, d] (16-byte aligned, d as above); starts int64 [n_groups + 1] ascending from 0 to
 *   n_members; members int32 [n_members] rows of src.  dst[g] float32 [n_groups, d] = the rows members[starts[g] :
 *   starts[g + 1]] added to +0 one after the other in list order, in float32 (an empty group: zeros).  No atomics: the
 *   bits are a function of the inputs.  A member outside [0, n_src) or a bad starts entry ORs bit 4 and is skipped
 *   (clamped).                                                                                                        */
int osn_merge_contacts(const int32_t* voxel_region, const int32_t* nbr, int64_t n_voxels, int connectivity,
                       int64_t n_regions, int64_t* key, int32_t* err, osn_stream_t stream);
int osn_rows_pair_dot(const void* rows_f16, int64_t n_rows, int d, const int32_t* lo, const int32_t* hi,
                      int64_t n_pairs, float* sim, int32_t* err, osn_stream_t stream);
size_t osn_merge_ws_bytes(int64_t n_regions);
int osn_merge_round(const int32_t* lo, const int32_t* hi, const float* sim, int64_t n_pairs, int64_t n_regions,
                    float threshold, int32_t* parent, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream);
int osn_rows_fold(const float* src, int64_t n_src, int d, const int64_t* starts, const int32_t* members,
                  int64_t n_members, int64_t n_groups, float* dst, int32_t* err, osn_stream_t stream);

/* ---- hash voxelisation --------------------------------------------------- *
 * Replaces Voxelizer.voxelize (dataset/voxelizer.py:117-129) +
 * sparse_quantize / fnv_hash_vec (dataset/voxelization_utils.py:9-22,112-132):
 *   grid = floor([xyz,1] @ T^T[:, :3]); grid -= min(grid); key = FNV64(grid)
 *   inds = first occurrence per distinct key in ascending key order,
 *   inverse[p] = rank of key(p).
 * xyz float64 [n,3] device; T12 = first three rows of the 4x4 transform, HOST,
 * row-major (12 doubles).  Outputs: grid_out float64 [n,3] (integral, shifted),
 * inds int64 [<=n], inverse int64 [n]; *n_vox_host on the HOST (one stream sync). */
size_t osn_voxelize_ws_bytes(int64_t n);
int osn_voxelize_fnv(const double* xyz, int64_t n, const double* T12_host,
                     double* grid_out, int64_t* inds, int64_t* inverse, int64_t* n_vox_host,
                     void* ws, size_t ws_bytes, osn_stream_t stream);
/* fnv_hash_vec alone (dataset/voxelization_utils.py:9-22): keys[i] of integral rows. */
int osn_fnv_hash(const double* grid, int64_t n, int ncol, uint64_t* keys, osn_stream_t stream);
/* ravel_hash_vec (dataset/voxelization_utils.py:25-41, the alternative key of sparse_quantize; the path itself
 * uses the FNV key): key = Fortran-style ravel of (coords - column minimum) over the column extents.
 * grid: float64 [n, ncol <= 4] integral values; ws: 128 bytes.                                              */
int osn_ravel_hash(const double* grid, int64_t n, int ncol, uint64_t* keys, void* ws, size_t ws_bytes,
                   osn_stream_t stream);

/* ---- loader-side batch assembly --------------------- *
 * Replaces the index1 / chunk_ind / cumsum chain of FusedFeatureLoader.__getitem__
 * (dataset/feature_loader.py:124-143; val/test :107-113,:166-171): after the voxeliser kept one
 * point per voxel (vox_ind = its `inds`), which voxels carry a fused 2-D feature and which row of
 * the compact feature matrix (one row per True of mask_chunk, in point order) belongs to each:
 *   mask_vox[v] = mask_chunk[vox_ind[v]]          uint8 [n_vox]
 *   src_row[v]  = #True in mask_chunk[0 .. vox_ind[v])  if mask_vox[v] else -1     int64 [n_vox]
 *   indices     = src_row[mask_vox] (voxel order kept; the reference's `indices`)  int64 [<= n_vox]
 * *n_sel_host = number of selected voxels, on the HOST (one stream sync).           */
size_t osn_feature_remap_ws_bytes(int64_t n_points, int64_t n_vox);
int osn_feature_remap(const uint8_t* mask_chunk, const int64_t* vox_ind, int64_t n_points, int64_t n_vox,
                      uint8_t* mask_vox, int64_t* src_row, int64_t* indices, int64_t* n_sel_host,
                      void* ws, size_t ws_bytes, osn_stream_t stream);
/* One scene's rows of the collated coordinate matrix (dataset/feature_loader.py:177-178,204-205):
 * out_coords4[i] = (batch_index, xyz3[i,0], xyz3[i,1], xyz3[i,2]); the caller passes the row offset
 * of the scene inside the batch tensor.                                             */
int osn_batch_coords(const int32_t* xyz3, int64_t n, int batch_index, int32_t* out_coords4,
                     osn_stream_t stream);

/* ---- multi-view feature fusion (the producer of the fused features the distillation trains on) ---- *
 * osn_fusion_project: scripts/feature_fusion/fusion_util.py:93-139 (PointCloudToImageMapper.compute_mapping).
 *   coords3 double [n, 3] (device); world_to_camera16 = np.linalg.inv(camera_to_world), row-major 4 x 4 (HOST);
 *   intrinsic4 = {fx, fy, cx, cy} (HOST); depth double [H, W] in metres (device) or NULL (then: in front of the camera);
 *   image is W x H pixels; cut_bound pixels of border are excluded; mapping int64 [n, 3] = (row, column, visible),
 *   zeros where not visible -- bit-identical to the numpy code (fp64, same operation order and rounding).
 * osn_fusion_accumulate: scripts/feature_fusion/scannet_openseg.py:93-106, one view: for visible points
 *   counter[p] += 1, sum_features[p, :] += feat2d[:, row, column]; feat2d float [D, H, W], sum float [n, D], counter float [n].
 * osn_fusion_finish: scannet_openseg.py:108-109: feat_bank = sum_features / (counter == 0 ? 1e-5 : counter).        */
int osn_fusion_project(const double* coords3, int64_t n, const double* world_to_camera16, const double* intrinsic4,
                       const double* depth, int H, int W, int cut_bound, double vis_thres, int64_t* mapping,
                       osn_stream_t stream);
int osn_fusion_accumulate(const float* feat2d, int D, int H, int W, const int64_t* mapping, int64_t n,
                          float* sum_features, float* counter, osn_stream_t stream);
int osn_fusion_finish(const float* sum_features, const float* counter, int64_t n, int D, float* feat_bank,
                      osn_stream_t stream);

/* ---- scene views: point-splat rasteriser with an exact z-buffer, and its shading pass (csrc/render.hip) ------------ *
 * The reference's headline is a picture -- the demo that highlights the regions matching a typed phrase -- and its
 * run/evaluate.py:343-376 exports coloured point clouds for an outside viewer; scripts/feature_fusion/nuscenes_openseg.py
 * calls compute_mapping with depth=None, so features bleed through walls.  One z-buffer serves both: pictures of any
 * per-point result, and a depth image rendered from the cloud itself for osn_fusion_project's occlusion test.
 *
 * osn_render_splat: coords3 double [n, 3] (device), n < 2^32 - 1; views20 (HOST) = n_views x (world_to_camera row-major
 *   4 x 4, then fx fy cx cy); image H x W, H * W < 2^31; radius (metres, finite, >= 0); max_px in 0 .. 16; near finite > 0;
 *   zbuf uint64 [n_views, H, W] (device).  zbuf is first filled with all ones (background).  Per (view, point):
 *     the camera-space point p and the rounded centre pixel (ur, vr) with exactly the arithmetic of osn_fusion_project
 *       (one shared body: csrc/project.h), so the centre is bit for bit the pixel compute_mapping gives;
 *     skipped unless p2 >= near (NaN fails), float32(p2) is finite, and |ur|, |vr| < 2^30 (NaN fails);
 *     r = 0 if radius == 0, else min(max_px, max(0, rint((radius * fx) / p2))) -- separate IEEE double multiply and
 *       divide, the clamp taken before the conversion to int (NaN gives 0);
 *     key = (uint64(bits of float32(p2), round to nearest) << 32) | point index;
 *     every pixel (ur + dx, vr + dy) with dx^2 + dy^2 <= r^2 inside the image takes the 64-bit unsigned atomic min of the
 *       key -- the footprint is clipped, a centre outside the image still draws what lies inside.
 *   The result is a pure function of the inputs whatever the schedule: the nearest float32 depth wins, equal depths go to
 *   the lower point index; two calls give the same bits.  One launch per view on `stream`, asynchronous, no workspace.
 *
 * osn_render_shade: zbuf [n_pixels] -> point_id int32 (-1 background), depth float32 (0 background: ScanNet's "no depth",
 *   which the occlusion test |d - p2| <= vis * d rejects), and rgb uint8 [n_pixels, 3] by mode (0: rgb is not written):
 *     1 colours  rgb = colors[id], colors uint8 [n, 3]
 *     2 labels   l = values[offset + id * stride] (int32: value_bytes 4, int64: 8); table = palette uint8 [table_rows, 3];
 *                rgb = table[l], or `other` when l is outside [0, table_rows)
 *     3 heat     h = values[offset + id * stride] (fp16: value_bytes 2, fp32: 4) -- one column of a [N, Q] heat-map in
 *                place; finite lo < hi; table = LUT uint8 [256, 3] (table_rows = 256).  NaN gives `other`; h < lo gives
 *                colors[id] when colors (the base image) is given, else table[0]; otherwise, with correctly rounded fp32
 *                operations, t = (float(h) - lo) / (hi - lo) and rgb = table[min(255, (int)rint(t * 255))].
 *   Background pixels get `background` in every mode; other_rgb / background_rgb are r | g << 8 | b << 16.  A point index
 *   >= n in zbuf is never dereferenced: the pixel gets `other`.  n < 2^31.  Integers and selected inputs only: exact.  */
int osn_render_splat(const double* coords3, int64_t n, const double* views20, int n_views, int H, int W, double radius,
                     int max_px, double near, uint64_t* zbuf, osn_stream_t stream);
int osn_render_shade(const uint64_t* zbuf, int64_t n_pixels, int64_t n, int32_t* point_id, float* depth, uint8_t* rgb,
                     int mode, const uint8_t* colors, const void* values, int value_bytes, int64_t value_offset,
                     int64_t value_stride, const uint8_t* table, int table_rows, float lo, float hi, uint32_t other_rgb,
                     uint32_t background_rgb, osn_stream_t stream);

/* ---- spatial neighbours on the voxel grid: k-nearest search, blend, vote (csrc/neighbors.hip) -------------------- *
 * Every application result is a tensor over the bank's own points; these entries move one to other points: into the rows
 * feature fusion never saw (run/evaluate.py:297-300), onto a foreign point set, or over a point's surroundings.
 * The err word (device int32, OR-ed into, never cleared here): 1 = an order entry outside [0, m), 2 = a cell column or a
 * table entry out of range, 4 = a cell's list range or point out of range, 8 = a neighbour index or count out of range.
 * Such entries are skipped, never dereferenced; the caller reads the word.  All calls are asynchronous on `stream`.
 *
 * osn_knn_grid: source xyz float32 [n, 3]; cell_start int32 [n_voxels + 1] and cell_points int32 [n_src]: the CSR of the
 *   source points per voxel row; nbr int32 [27, n_cells] (-1 absent): the voxel rows around each cell column; per query
 *   q < m its query_xyz float32 [m, 3], its column q_cell (-1: invalid, no neighbours), its exclude (a point never
 *   returned; the array may be null) and its place in `order` (null: row order), the sequence the lanes take the queries
 *   in -- cell order keeps a wave on the same lists; it must be a permutation of 0 .. m - 1 (a query it does not name is
 *   not written).  1 <= k <= 16; r2 finite >= 0.
 *   Candidates: the points cell_points[cell_start[v] .. cell_start[v + 1]) of the 27 rows v = nbr[o, q_cell[q]] >= 0,
 *   without exclude[q].  dx = q.x - p.x (dy, dz alike), d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), separately rounded
 *   float32 operations; kept when d2 <= r2 (NaN fails).  key = bits(d2) << 32 | point index; the k smallest keys ascending
 *   -> idx int32 [m, k] (-1 past count), dist2 float32 [m, k] (+inf past count), count int32 [m].  A pure function of the
 *   inputs whatever the schedule; two calls give the same bits.
 * osn_knn_blend: values fp16 (value_bytes 2) or fp32 (4) [n, n_cols], n_cols >= 1; per query over j < count in ascending
 *   j: w_j = 1 (inverse == 0) or 1 / (dist2_j + eps); out = (w_0 v_0 + w_1 v_1 + ...) / (w_0 + w_1 + ...), every product,
 *   sum and the divide one float32 rounding, the result rounded once to the values' type; the sums start at their first
 *   term, so k = 1 uniform copies the row bit for bit.  count == 0: out = fill, found = 0 (found uint8 [m]).
 * osn_knn_vote: labels int64 [n]; negative labels are ignored; out int64 [m] = the label most of the count neighbours
 *   hold, a tie going to the label whose first holder has the smallest j; `fill` without a non-negative label.  Exact. */
int osn_knn_grid(const float* xyz, int64_t n, const int32_t* cell_start, const int32_t* cell_points, int64_t n_src,
                 int64_t n_voxels, const int32_t* nbr, int64_t n_cells, const float* query_xyz, const int32_t* q_cell,
                 const int32_t* exclude, const int32_t* order, int64_t m, int k, float r2, int32_t* idx, float* dist2,
                 int32_t* count, int32_t* err, osn_stream_t stream);
int osn_knn_blend(const void* values, int value_bytes, int64_t n, int64_t n_cols, const int32_t* idx, const float* dist2,
                  const int32_t* count, int64_t m, int k, int inverse, float eps, float fill, void* out, uint8_t* found,
                  int32_t* err, osn_stream_t stream);
int osn_knn_vote(const int64_t* labels, int64_t n, const int32_t* idx, const int32_t* count, int64_t m, int k, int64_t fill,
                 int64_t* out, int32_t* err, osn_stream_t stream);

/* ---- nearest sources at any range: exact distance fields on the voxel grid (csrc/reach.hip) ---------------------- *
 * osn_knn_grid stops one voxel from the query.  This entry finds, for every query cell, the nearest source cell of the
 * same scene inside a Euclidean ball of `reach` cells (1 .. 4096), exactly: cells are integers, so is
 * d2 = dx dx + dy dy + dz dz, and the result is the minimum of ONE 64-bit key,  uint32(d2) << 32 | uint32(id),  over the
 * candidates -- the sources of the query's scene with |dx|, |dy|, |dz| <= reach and d2 <= reach^2.  A tie in d2 goes to
 * the lowest id; a query that is itself a source gets d2 = 0.  No floating point, no atomics across workgroups: a pure
 * function of the inputs whatever the schedule, two calls give the same bits.  Cells lie in the packable range
 * |c| < 32767; a difference reaches 65 532 and its square does not fit 32 bits, so an axis is rejected by |d| > reach
 * before any square is formed and no wrapped value is compared.
 *
 * osn_reach_nearest takes SORTED data (openscene_amd.ops.reach_nearest does the sorting in torch); block = cell >> 3 per
 * axis (arithmetic shift: a floor division), ids >= 0:
 *   q_cells int32 [n_queries, 4] rows (scene, x, y, z) sorted by (scene, block); order int32 [n_queries] (null: identity):
 *     the result of sorted query i goes to row order[i] of the outputs;
 *   src int32 [n_src, 4] rows (x, y, z, id) sorted by (scene, block); blocks int32 [n_blocks, 4] rows (scene, bx, by, bz):
 *     the occupied blocks in that order; block_start int32 [n_blocks + 1]: block b holds src[block_start[b] ..
 *     block_start[b + 1]): 512 entries for 8^3 distinct cells (repeated cells are allowed; LDS holds 512 at a time);
 *   items int32 [n_items, 4] rows (q_start, q_end, block_start, block_end): at most 256 consecutive sorted queries of ONE
 *     scene and the range of that scene's rows in `blocks`.  One workgroup per item, one query per lane: it walks the
 *     range, first the blocks that touch the bounding box of its queries, then the others; it skips a block whose gap to
 *     the box exceeds reach on an axis, or whose squared gap exceeds the largest best d2 of its lanes so far (a block at
 *     exactly that bound is visited: it may hold a lower id); it stages a visited block in LDS and every lane scans it.
 *   q_cells, items, src and blocks are 16-byte aligned.
 * -> dist2 int32 [n_queries] and nearest int32 [n_queries] (the id), both -1 without a candidate; a query no item names
 * is not written.  The err word (device int32, OR-ed into, never cleared here): 1 = an item's ranges out of range, 2 = a
 * block's entry range or coordinates out of range, 4 = a cell outside the packable range, 8 = an order entry outside
 * [0, n_queries).  Such entries are skipped, never dereferenced.  Asynchronous on `stream`, no workspace.              */
int osn_reach_nearest(const int32_t* q_cells, const int32_t* order, int64_t n_queries, const int32_t* items, int64_t n_items,
                      const int32_t* src, int64_t n_src, const int32_t* blocks, const int32_t* block_start, int64_t n_blocks,
                      int reach, int32_t* dist2, int32_t* nearest, int32_t* err, osn_stream_t stream);

/* ---- two scans in one frame: rigid RANSAC over correspondences, moments for Kabsch / ICP (csrc/align.hip) --------- *
 * Pairs are src, dst float32 [n_pairs, 3] on the device: pair p says "point src[p] of one scan is point dst[p] of the
 * other" (openscene_amd.match.mutual gives the rows).  A transform is 12 float32: R row-major, then t; it takes src onto
 * dst.  THE RESIDUAL of a pair under a transform is, in float32, every operation rounded on its own (no FMA):
 *     x_i = ((R_i0 s_0) + (R_i1 s_1)) + (R_i2 s_2)     e_i = (x_i + t_i) - d_i     r2 = ((e_0 e_0) + (e_1 e_1)) + (e_2 e_2)
 * and the pair is an INLIER iff r2 <= tau2 (a NaN never is); tau2 = float32(threshold) * float32(threshold), rounded once
 * by the caller.  numpy float32 gives the same bits, so counts and masks are exact.  All calls are asynchronous on
 * `stream`, allocate nothing and use no floating-point atomics; n_pairs < 2^31, n_hyp <= OSN_RIGID_MAX_HYPOTHESES.
 *
 * osn_rigid_from_triplets: triplets int32 [n_hyp, 3] (device) name three pairs each; xf float32 [n_hyp, 12] and valid
 *   uint8 [n_hyp] receive the motion that takes the src triangle onto the dst triangle.  With p0, p1, p2 widened to
 *   float64 and every float64 operation rounded on its own, in this order:
 *     a = p1 - p0, b = p2 - p0, c = p2 - p1;  |v|^2 = ((v0 v0) + (v1 v1)) + (v2 v2), |v| = sqrt(|v|^2);
 *     u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0);  e1 = a / |a|, n = a x b, e3 = n / |n|, e2 = e3 x e1;
 *     R_ij = ((e1d_i e1s_j) + (e2d_i e2s_j)) + (e3d_i e3s_j)               (F_dst F_src^T, F = [e1 e2 e3] as columns)
 *     t_i = d0_i - (((R_i0 s0_0) + (R_i1 s0_1)) + (R_i2 s0_2))             (with the float64 R)
 *   R and t are rounded to float32 once, at the end.  A hypothesis is INVALID -- valid = 0, R = identity, t = 0 -- when
 *   an index lies outside [0, n_pairs) or two are equal (such rows are never dereferenced); when not |n|^2 > area2_min
 *   for either triangle (NaN fails); or when not | |v|_src - |v|_dst | <= 2 * threshold for any of the sides a, b, c (the
 *   congruence pre-test: a triplet that holds an outlier rarely passes it).  threshold, area2_min finite and >= 0.
 * osn_rigid_score: counts int32 [n_hyp] = the number of inliers of every hypothesis of xf float32 [n_hyp, 12] (16-byte
 *   aligned); -1 where valid (uint8 [n_hyp]; null: all valid) is 0.  n_hyp * n_pairs residuals, no temporary: the grid is
 *   (tiles of 1024 pairs) x (tiles of 64 hypotheses), the counts are integer atomics (exact, order-free) on a `counts`
 *   this call initialises.  The contract forbids FMA: 21 VALU operations per residual where a fused form takes 15.
 * osn_rigid_best: best int32 [2] (device) = (the largest count, the lowest hypothesis that has it), the maximum of one
 *   64-bit key (count with its sign bit flipped) << 32 | ~h.  n_hyp >= 1.
 * osn_rigid_moments: under ONE transform xf12 (12 floats in HOST memory, read during the call): pair i is (src[i],
 *   dst[i]) or, with dst_idx int32 [n_pairs] (the ICP form: a neighbour list, no gathered copy of dst), (src[i],
 *   dst[dst_idx[i]]); dst float32 [n_dst, 3]; an index < 0 or >= n_dst means no partner and is never dereferenced
 *   (without dst_idx n_dst >= n_pairs).  Writes inlier uint8 [n_pairs] and r2 float32 [n_pairs] as defined above (no
 *   partner: 0 and +inf) and moments double [16] (device) over the inliers: n, sum s (3), sum d (3), sum s d^T (9,
 *   row-major s_i d_j).  float64; a product of two float32 is exact, the additions run in a fixed order -- chunks of
 *   OSN_RIGID_MOMENTS_CHUNK pairs, each reduced in a fixed tree, the chunk partials added in ascending chunk order -- so
 *   two calls give the same bits.  ws: osn_rigid_moments_ws_bytes(n_pairs) bytes, 16-byte aligned.                      */
#define OSN_RIGID_MAX_HYPOTHESES (1 << 20)
#define OSN_RIGID_MOMENTS_CHUNK 1024
int osn_rigid_from_triplets(const float* src, const float* dst, int64_t n_pairs, const int32_t* triplets, int n_hyp,
                            float threshold, double area2_min, float* xf, uint8_t* valid, osn_stream_t stream);
int osn_rigid_score(const float* src, const float* dst, int64_t n_pairs, const float* xf, const uint8_t* valid, int n_hyp,
                    float tau2, int32_t* counts, osn_stream_t stream);
int osn_rigid_best(const int32_t* counts, int n_hyp, int32_t* best, osn_stream_t stream);
size_t osn_rigid_moments_ws_bytes(int64_t n_pairs);
int osn_rigid_moments(const float* src, const float* dst, const int32_t* dst_idx, int64_t n_pairs, int64_t n_dst,
                      const float* xf12_host, float tau2, uint8_t* inlier, float* r2, double* moments, void* ws,
                      size_t ws_bytes, osn_stream_t stream);

/* ---- elastic distortion: the pre-voxeliser transform of Point3DLoader (dataset/point_loader.py:156) ---------- *
 * ElasticDistortion.elastic_distortion (dataset/augmentation.py:159-201), bit-identical to numpy / scipy given the
 * same noise draw; the draw (np.random.randn(*noise_dim, 3).astype(float32)) and np.linspace of the axes stay on the host.
 * osn_bbox: bbox6 (device, 6 doubles) = per-axis min of xyz float64 [n,3], then per-axis max.  n >= 1.
 * osn_elastic_blur: in place on noise float32 [nx, ny, nz, 3]: the six scipy.ndimage.convolve passes (3-tap box of
 *   weight (double)(float)(1/3) along x, y, z, twice; zero boundary; double accumulation, float32 after each pass).
 * osn_elastic_apply: out = xyz + RegularGridInterpolator(axes, noise, bounds_error=0, fill_value=0)(xyz) * magnitude
 *   (scipy's linear rule and operation order), and bbox6 = the bounding box of out (sizes the next field).
 *   axes float64 [nx + ny + nz] (device, ascending, >= 2 nodes each); out must not alias xyz.                    */
size_t osn_bbox_ws_bytes(int64_t n);
int osn_bbox(const double* xyz, int64_t n, double* bbox6, void* ws, size_t ws_bytes, osn_stream_t stream);
size_t osn_elastic_blur_ws_bytes(int nx, int ny, int nz);
int osn_elastic_blur(float* noise, int nx, int ny, int nz, void* ws, size_t ws_bytes, osn_stream_t stream);
size_t osn_elastic_apply_ws_bytes(int64_t n);
int osn_elastic_apply(const double* xyz, int64_t n, const float* noise, int nx, int ny, int nz, const double* axes,
                      double magnitude, double* out, double* bbox6, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- network executor: one call per forward / backward pass of a MinkUNet -------------------------------- *
 * Replaces the Python-level walk of models/mink_unet.py:116-174 (MinkUNetBase.forward: conv0 .. block8, final) and
 * of its autograd graph.  The module tree is compiled ONCE into a linear program of stages
 *   x = conv(src)  [-> BN (batch or running statistics) (+ residual) (+ ReLU)]  -> dst  [-> second store into a cat buffer]
 * and the library issues every launch of a pass from one call: kernel choice per stage, scratch, the training-mode
 * statistics kept for the backward pass, the gradient routing (sums of up to three sources are formed inside the
 * batch-norm backward, ME.cat is written in place by its producers).  Same kernels and same results as the per-module
 * entry points above; what disappears is the host work between launches (~40 us per stage of Python + autograd).
 * All `const T*` members of the descriptors are HOST arrays unless noted; activations live in caller-provided arenas. */
#define OSN_NET_MAX_LEVELS 8
typedef struct osn_net_op {
    int32_t K, cin, cout;        /* kernel volume (1, 8, 27, 125), channels                                      */
    int32_t lvl_in, lvl_out;     /* pyramid levels (index into level_rows) of the input / output rows           */
    int32_t map;                 /* index into osn_net_run.maps, -1 <=> K == 1 (identity map)                     */
    int32_t transposed;          /* 1: MinkowskiConvolutionTranspose (runs on the mirrored tables of `map`)       */
    int32_t src;                 /* activation buffer read, -1 = the network input                                */
    int32_t dst;                 /* activation buffer written, -1 = the network output (no batch norm: `final`)   */
    int32_t bn;                  /* index into osn_net_run.bns, -1 = none                                         */
    int32_t relu;                /* ReLU after the batch norm (+ residual)                                        */
    int32_t res;                 /* residual buffer added before the ReLU, -1 = none                              */
    int32_t copy_buf, copy_col;  /* second store of dst: columns [copy_col, copy_col + cout) of buffer copy_buf   */
    int32_t weight;              /* index into osn_net_run.weights                                                */
    int32_t need_dgrad;          /* 0: the input needs no gradient (stem)                                         */
    int32_t fine_unique;         /* 1: `map` is a 2^3 stride-2 map -- every row of its fine side has exactly one pair
                                  *    (osn_spconv_fwd_ws direct mode for the launches that write the fine side)   */
    int32_t reserved;
} osn_net_op;                    /* 72 bytes */
typedef struct osn_net_buf { int32_t level, channels; } osn_net_buf;
typedef struct osn_net_desc {
    int32_t n_ops, n_bufs, n_bns, n_weights, n_maps, n_levels;
    int32_t tl_min_rows;         /* tile-list forward / input gradient on tables of at least this many rows       */
    int32_t tl_mid_rows;         /* ... and from this many rows on when both channel counts are >= 96 (0 = never)  */
    int32_t ws_max_rows;         /* weight-stationary kernel (osn_spconv_fwd_ws) for launches writing at most this
                                  *    many rows (0 = never; the direct mode of fine_unique maps is not limited)   */
    int32_t reserved;
    const osn_net_op* ops;
    const osn_net_buf* bufs;
} osn_net_desc;
enum { OSN_NET_K_NONE = 0, OSN_NET_K_STEM = 1, OSN_NET_K_TL = 2, OSN_NET_K_X6 = 3, OSN_NET_K_WGRAD_TL = 4, OSN_NET_K_WGRAD = 5,
       OSN_NET_K_WS = 6, OSN_NET_K_WS_DIRECT = 7, OSN_NET_K_WGRAD_STEM = 8, OSN_NET_K_DENSE = 9, OSN_NET_K_RG = 10 };
enum { OSN_NET_IMG_X6_FWD = 1, OSN_NET_IMG_X6_DGRAD = 2, OSN_NET_IMG_TL_FWD = 4, OSN_NET_IMG_TL_DGRAD = 8 };
typedef struct osn_net_plan {                 /* every array is caller-provided HOST memory                       */
    uint64_t fwd_arena_bytes, bwd_arena_bytes, ws_bytes;
    uint64_t* x_off;             /* [n_ops]  conv output (pre batch norm) in the forward arena                    */
    uint64_t* stat_off;          /* [n_ops]  mean | var (2 x cout floats) of the training-mode statistics          */
    uint64_t* y_off;             /* [n_bufs] activation buffers in the forward arena                              */
    int32_t* fwd_kernel;         /* [n_ops]  OSN_NET_K_*                                                          */
    int32_t* dgrad_kernel;       /* [n_ops]                                                                       */
    int32_t* wgrad_kernel;       /* [n_ops]                                                                       */
    int32_t* images;             /* [n_ops]  OSN_NET_IMG_* bit mask of the weight images the pass reads            */
} osn_net_plan;
typedef struct osn_net_map {                  /* one kernel map of the coordinate manager (device pointers)       */
    const int32_t* nbr_fwd;      /* [K, rows_out]                                                                 */
    const int32_t* nbr_bwd;      /* [K, rows_in] table of the input gradient (= nbr_fwd for odd stride-1 kernels)  */
    const int32_t* tiles_fwd_rows; const int32_t* tiles_fwd_tbl; const uint32_t* tiles_fwd_gmask;   /* osn_kmap_sort, or null */
    const int32_t* tiles_bwd_rows; const int32_t* tiles_bwd_tbl; const uint32_t* tiles_bwd_gmask;
    const int64_t* counts;       /* [K] pairs per offset                                                          */
    const void* tl_fwd; const int32_t* tl_fwd_rows;     /* osn_tile_lists_build of the forward table (+ permutation) */
    const void* tl_bwd; const int32_t* tl_bwd_rows;
    const void* pl_fwd;          /* osn_pair_lists_build of tl_fwd: weight gradient, weight-stationary convolutions  */
    int32_t K, flip, tl_fwd_bm, tl_bwd_bm;
} osn_net_map;
typedef struct osn_net_weight {
    const float* W;              /* [K, cin, cout]                                                                */
    const void* x6_fwd; const void* x6_dgrad; const void* tl_fwd; const void* tl_dgrad;    /* images (OSN_NET_IMG_*) */
    float* gW;                   /* backward: receives the weight gradient                                        */
} osn_net_weight;
typedef struct osn_net_bn {
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;
    float* ggamma; float* gbeta; /* backward                                                                      */
    float eps, momentum;
} osn_net_bn;
typedef struct osn_prof osn_prof_t;           /* optional launch timer, see osn_prof_create                       */
typedef struct osn_events osn_events_t;       /* pool of HIP events for the fork / join of the backward pass      */
/* osn_net_run.flags.  NO_JOIN (backward pass with a side stream, a call that is NOT the last segment of the pass): return
 * without making `stream` wait for the side stream.  The weight gradients of the executed ops are then final in SIDE-stream
 * order only -- a consumer (the gradient exchange of a segmented pass) must queue behind the side stream; the call that
 * plays the last segment (flags 0) joins everything.  Input gradients a later segment reads are joined by their own events
 * either way.                                                                                                      */
#define OSN_NET_RUN_NO_JOIN 1
/* osn_net_forward, evaluation mode: by default a stage's batch norm (+ residual) (+ ReLU) (+ cat store) is applied in the EPILOGUE of
 * the kernel that finishes the stage's convolution (csrc/epilogue.h: same expression, bitwise the separate launch); this flag keeps
 * the separate osn_bn_apply launch (A/B, tests).                                                                          */
#define OSN_NET_RUN_NO_BN_EPILOGUE 2
/* osn_net_forward, evaluation mode only: the reduced-precision modes of the `_pieces` entries above for EVERY convolution launch of
 * the tile-list, register-gather, weight-stationary and 1x1 families (epilogue instances included); the stem and the first-generation
 * kernel stay exact.  Both bits, either bit with run.training != 0, and either bit in osn_net_backward: OSN_E_ARG before the first
 * launch.  osn_net_plan_query does not know the mode: arenas and workspaces are those of the exact pass.                       */
#define OSN_NET_RUN_PIECES_2 4
#define OSN_NET_RUN_PIECES_1 8
/* Reduced-precision TRAINING: accepted by osn_net_forward (any run.training) and by osn_net_backward.  With one of them set every
 * launch of the same four families in that call -- forward launches; in osn_net_backward their input-gradient launches (the head's
 * row-compacted one included) and every OSN_NET_K_WGRAD_TL weight gradient (osn_spconv_wgrad_tl_partial_pieces) -- runs with two /
 * one pieces.  The stem (forward and weight gradient), the first-generation kernels (osn_spconv_fwd_x6, osn_spconv_wgrad), batch
 * norm and everything else stay exact; parameters, gradients and partial sums stay fp32.  A pass's forward and backward calls
 * (every segment of a segmented backward pass) should carry the same bit.  With a bit set osn_net_backward adds the three gradient
 * sources of a tensor with three consumers last consumer first (autograd's order: the module-by-module path then gives the same bits;
 * without a bit the order is first consumer first, as it always was).  Both bits, or one of them together with
 * OSN_NET_RUN_PIECES_2 / _1: OSN_E_ARG before the first launch.  osn_net_plan_query does not know the mode.                     */
#define OSN_NET_RUN_TRAIN_PIECES_2 16
#define OSN_NET_RUN_TRAIN_PIECES_1 32
typedef struct osn_net_run {
    const int64_t* level_rows;   /* [n_levels] rows of every pyramid level                                        */
    const osn_net_map* maps;
    const osn_net_weight* weights;
    const osn_net_bn* bns;
    const float* input;          /* [rows(level of op 0), cin of op 0]                                            */
    float* output;               /* forward: [rows, cout] of the op with dst == -1 (may be null if not run)       */
    const float* goutput;        /* backward: gradient of `output`; may be null when goutput_rows (below) carries every
                                  * non-zero row of it -- the head then ran on those rows only (round 6)               */
    void* fwd_arena; uint64_t fwd_arena_bytes;
    void* bwd_arena; uint64_t bwd_arena_bytes;
    void* ws; uint64_t ws_bytes;
    int32_t* tl_counters;        /* 128 persistent tile counters of this stream (osn_spconv_fwd_tl counters)      */
    int32_t training;            /* batch statistics + running update (1) or running statistics (0)               */
    int32_t first_op, end_op;    /* ops [first_op, end_op) are executed                                           */
    int32_t flags;               /* OSN_NET_RUN_*                                                                 */
    osn_prof_t* prof;            /* nullable                                                                      */
    /* all nullable: work that is off the main dependency chain runs on `side_stream` -- in both passes the BasicBlock
     * shortcut stages (1x1 conv + batch norm, beside conv1 - BN - conv2), in the backward pass also every weight
     * gradient (needed only at the end of the pass).  The passes fork and join with events of `events`, so nothing
     * outside sees the second stream; results are bitwise those of a single stream.                               */
    osn_stream_t side_stream;
    void* ws_side; uint64_t ws_side_bytes;     /* scratch of the side stream's launches (same size rule as ws)       */
    osn_events_t* events;        /* osn_events_create(2 * n_ops + 2)                                              */
    /* backward, all nullable: `goutput` is zero outside `n_grows` rows (the distillation loss supervises ~20 % of the
     * voxels: run/distill.py:321-326 indexes the output with a mask before the loss, so autograd's gradient of the full
     * output has zero rows everywhere else).  grows_pos[r] = j for the j-th such row, -1 otherwise (osn_distill_loss_* keeps
     * it); grows_idx[j] = r; goutput_rows [n_grows, cout] = goutput[grows_idx].  Given all three, the input and weight
     * gradients of the op that produced `output` run on the n_grows rows only (same values: the other rows contribute
     * exact zeros).                                                                                                */
    const int32_t* grows_pos;
    const int64_t* grows_idx;
    const float* goutput_rows;
    int64_t n_grows;
} osn_net_run;
int osn_net_plan_query(const osn_net_desc* net, const int64_t* level_rows, int training, osn_net_plan* plan);
/* out[j, :] = in[idx[j], :] (c % 4 == 0) and its inverse out[r, :] = pos[r] >= 0 ? in[pos[r], :] : 0 over all n rows: the row
 * compaction around the head's gradients (`output_3d[mask]`, run/distill.py:322, and torch's index backward)        */
int osn_rows_gather(const float* in, const int64_t* idx, int64_t n_idx, int c, float* out, osn_stream_t stream);
int osn_rows_scatter_zero(const float* in, const int32_t* pos, int64_t n, int c, float* out, osn_stream_t stream);
int osn_net_forward(const osn_net_desc* net, const osn_net_run* run, osn_stream_t stream);
int osn_net_backward(const osn_net_desc* net, const osn_net_run* run, osn_stream_t stream);
osn_events_t* osn_events_create(int n);       /* n timing-free HIP events on the current device; null on failure   */
void osn_events_destroy(osn_events_t* e);

/* ---- every kernel map of a scene from one call ------------------------------------------------------- *
 * Replaces the per-map calls behind [ME] CoordinateManager.kernel_map for the convolutions of one forward pass
 * (models/mink_unet.py:47-113: a 5^3 map, five 3^3 maps, four 2^3 stride-2 maps + their transposes).  A job = one map
 * with everything derived from it; null output pointers skip a product.  Jobs name the stream they run on (index into
 * `streams`, [0] = the caller's stream): the maps of different levels are independent chains of latency-bound launches,
 * so they run side by side; the call forks after what is queued on streams[0] (the coordinate pyramid) and joins before
 * it returns.  ws[s] = scratch of stream s (osn_kmap_sort_ws_bytes of the largest table sorted there).  Tables are bit
 * for bit those of osn_kmap_build[_self] / osn_kmap_transpose / osn_kmap_sort / osn_tile_lists_build / osn_pair_lists_build. */
#define OSN_MAPS_MAX_STREAMS 4
typedef struct osn_map_level {               /* one pyramid level (osn_coords_unique[_async])                     */
    const int32_t* coords4; const uint64_t* keys; const int32_t* vals;
    int64_t cap, rows;
} osn_map_level;
typedef struct osn_map_job {
    int32_t lvl_in, lvl_out;     /* table of lvl_in probed at the coordinates of lvl_out                          */
    int32_t ksize, scale;        /* kernel size, offset scale (dilation x tensor stride of the input map)         */
    int32_t self_map;            /* 1: odd kernel over the table's own rows (osn_kmap_build_self; no nbr_bwd)     */
    int32_t stream;              /* index into `streams`                                                          */
    int32_t bm_fwd, bm_bwd;      /* tile rows of the lists (osn_tile_rows)                                        */
    int32_t* nbr_fwd; int32_t* nbr_bwd; int64_t* counts;
    int32_t* order_fwd; int32_t* sorted_fwd; uint32_t* gmask_fwd;
    int32_t* order_bwd; int32_t* sorted_bwd; uint32_t* gmask_bwd;
    void* tl_fwd; void* tl_bwd; void* pl_fwd;
} osn_map_job;                               /* 128 bytes */
int osn_maps_build(const osn_map_level* levels, int n_levels, const osn_map_job* jobs, int n_jobs,
                   const osn_stream_t* streams, void* const* ws, const uint64_t* ws_bytes, int n_streams,
                   osn_events_t* events);
/* osn_maps_build with block occupancy: occ[l] (nullable, as the array itself) = a buffer of osn_maps_occupancy_bytes(rows of level
 * l) bytes, 8-byte aligned.  A level that has one gets a second hash table over the 4^3 blocks of its cells (one 64-bit word of cell
 * bits per block; one launch in front of the level's first probed 3^3 / 5^3 self map, on its stream), and such self maps look up the
 * block words around a row and probe the coordinate table only where a cell is occupied -- a scene is a surface, most cells of a 5^3
 * neighbourhood are empty.  The rows of the level must be multiples of the job's `scale` for this to pay (the kernel finds out and
 * otherwise probes every offset).  Same tables, bit for bit.                                                                   */
size_t osn_maps_occupancy_bytes(int64_t rows);
int osn_maps_build_occ(const osn_map_level* levels, int n_levels, const osn_map_job* jobs, int n_jobs,
                       const osn_stream_t* streams, void* const* ws, const uint64_t* ws_bytes, int n_streams,
                       osn_events_t* events, void* const* occ);
/* By default a 3^3 self map that follows a 5^3 self map of the same level and scale in `jobs` is copied out of the finished 5^3
 * table (27 of its 125 offset rows, and their counts) on the 5^3 job's stream -- no hash probe, no preset -- and
 * osn_pair_lists_build plans the work items in workgroup 0 of its fill launch.  Tests and A/B only, process-wide: on != 0 runs
 * the earlier launch sequence (every self map probed at every offset, occ ignored, pair_plan_kernel a launch of its own).  Every
 * product is bit for bit the same either way.  Returns the previous setting.                                                 */
int osn_maps_set_legacy(int on);

/* Launch timer for the executor (bench.py's roofline entry): HIP events recorded on the launch stream around the
 * convolution launches of selected stages.  tag = op * 4 + phase (0 forward, 1 input gradient, 2 weight gradient).
 * osn_prof_filter: bracket only the listed tags (HOST array; n_tags = 0: every launch).  osn_prof_read synchronises
 * the events and returns the number of records (tags / ms: HOST arrays of `capacity` entries).                     */
osn_prof_t* osn_prof_create(int capacity);
void osn_prof_destroy(osn_prof_t* p);
int osn_prof_filter(osn_prof_t* p, const int32_t* tags, int n_tags);
int osn_prof_read(osn_prof_t* p, int32_t* tags, float* ms, int capacity, int reset);

/* ---- sparse pooling layers ---------------------------------------------------------------------------- *
 * [ME] MinkowskiSumPooling / MinkowskiAvgPooling / MinkowskiMaxPooling, MinkowskiGlobal{Sum,Avg,Max}Pooling and
 * MinkowskiBroadcast{Addition,Multiplication}: the layers models/resnet_base.py:54,69,71 builds next to its convolutions
 * (glob_avg = ME.MinkowskiGlobalMaxPooling(), MinkowskiAvgPooling, final = ME.MinkowskiLinear).  Semantics recalled from ME
 * v0.5.4.  Features are float32 [rows, c], any c >= 1: 16-byte accesses when c % 4 == 0 and every
 * matrix is 16-byte aligned, one element per thread otherwise.  No floating-point atomics anywhere: every result is a pure
 * function of the arguments, bit for bit repeatable.  Every refused argument of this family -- a null pointer, K or mode out of
 * range, a workspace below osn_gpool_ws_bytes -- returns OSN_E_ARG before anything is launched, the entry's name first in the text. */
#define OSN_POOL_SUM 0
#define OSN_POOL_AVG 1
#define OSN_POOL_MAX 2
#define OSN_GPOOL_CHUNK 512      /* rows of a batch that are reduced into one fp32 partial                              */
#define OSN_BROADCAST_ADD 0
#define OSN_BROADCAST_MUL 1
/* Local pooling over a kernel map (models/resnet_base.py:54,69,71; the table of osn_kmap_build: nbr[k, o] = input row or -1,
 * an entry outside [0, n_in) counts as absent), K = 8 (a 2^3 kernel) or 27 (3^3).
 *   osn_pool_count  cnt[o] = present neighbours of output row o (the divisor of avg; kept next to the map).
 *   osn_pool_fwd    sum: y[o] = fp32 sum of x[nbr[k, o]] over the present k, added one by one in ascending k from +0;
 *                   avg: that sum / float(cnt[o]) (IEEE division; no neighbour: 0);
 *                   max: the maximum, arg[o, c] = its input row (int32; -1 and y = 0 without a neighbour); ties to the lowest k
 *                   (+0 == -0), a NaN wins and the first NaN in k order stays.  `arg` is read for max only.
 *   osn_pool_bwd    gx[i] = sum over the forward offsets k = 0 .. K - 1, in that order, of the term of the output row
 *                   o = nbr_bwd[k, i] (the table of osn_kmap_transpose; flip = 1: the forward table of an odd stride-1 kernel
 *                   itself, forward offset k at row K - 1 - k):  gy[o]  |  gy[o] / float(cnt[o])  |  arg[o, c] == i ? gy[o, c] : 0. */
int osn_pool_count(const int32_t* nbr, int64_t n_in, int64_t n_out, int K, int32_t* cnt, osn_stream_t stream);
int osn_pool_fwd(const float* x, int64_t n_in, const int32_t* nbr, int64_t n_out, int K, int c, int mode, float* y, int32_t* arg,
                 osn_stream_t stream);
int osn_pool_bwd(const float* gy, int64_t n_out, const int32_t* nbr_bwd, int64_t n_in, int K, int flip, int c, int mode,
                 const int32_t* cnt, const int32_t* arg, float* gx, osn_stream_t stream);
/* Global pooling (models/resnet_base.py:54,69,71: glob_avg): y[b] = reduce over the rows order[offsets[b] .. offsets[b + 1]) of x,
 * `order` the rows of every batch in ascending row index (int32 [n]), `offsets` int64 [n_batches + 1].  A batch's list is cut into
 * chunks of OSN_GPOOL_CHUNK entries; a chunk is reduced in an order that depends on c alone, the partials are added in chunk
 * order, avg then divides once by float(n_b): a batch's bits depend on its own rows only.  max: exact, arg[b, c] = the lowest
 * row among equals (+0 == -0), a NaN wins and arg is the lowest NaN row; an empty batch gives 0 (sum, avg) or -inf and arg -1.
 * osn_gpool_bwd: rank[i] = batch position of row i (int32 [n]);  gx[i] = gy[rank[i]]  |  gy[rank[i]] / float(n_b)  |
 * arg[rank[i], c] == i ? gy[rank[i], c] : 0; every element of gx is written.                                              */
size_t osn_gpool_ws_bytes(int64_t n, int64_t n_batches, int c);
int osn_gpool_fwd(const float* x, int64_t n, int c, const int32_t* order, const int64_t* offsets, int64_t n_batches, int mode,
                  float* y, int32_t* arg, void* ws, size_t ws_bytes, osn_stream_t stream);
int osn_gpool_bwd(const float* gy, const int32_t* rank, const int64_t* offsets, const int32_t* arg, int64_t n, int64_t n_batches,
                  int c, int mode, float* gx, osn_stream_t stream);
/* Broadcast of a pooled tensor over the rows of its batches (the squeeze-excite gate on a models/resnet_base.py:54,69,71 trunk):
 * y[i] = x[i] + g[rank[i]]  (op 1: *), one streaming pass; the input gradient of a multiplication is the same call on gy.
 * osn_broadcast_bwd_pooled: gg[b] = sum over the batch's rows of gy[i]  (x != null: gy[i] * x[i], formed where the row is read),
 * through the chunked reduction of osn_gpool_fwd (workspace: osn_gpool_ws_bytes).                                           */
int osn_broadcast_fwd(const float* x, const float* g, const int32_t* rank, int64_t n, int64_t n_batches, int c, int op, float* y,
                      osn_stream_t stream);
int osn_broadcast_bwd_pooled(const float* gy, const float* x, int64_t n, int c, const int32_t* order, const int64_t* offsets,
                             int64_t n_batches, float* gg, void* ws, size_t ws_bytes, osn_stream_t stream);

/* ---- points in and out of the voxel grid (csrc/field.hip) ------------------------------------------------ *
 * [ME] TensorField / .sparse(), SparseTensor.slice(), SparseTensor.interpolate(), MinkowskiInterpolation and
 * features_at_coordinates, where run/evaluate.py:283-292 hands a point the row of its voxel (predictions[inds_reverse]).
 * Semantics recalled from ME v0.5.4.  Features are float32 [rows, c], any c >= 1: 16-byte accesses when
 * c % 4 == 0 and the matrices are 16-byte aligned, one element per thread otherwise.  Every float32 operation rounds on its own
 * (no FMA contraction) and there are no floating-point atomics: every result is a pure function of the arguments, bit for bit
 * repeatable.  Every refused argument -- a null pointer, c < 1, a stride below 1, a negative size, 8 m past the int32 pair index --
 * returns OSN_E_ARG before anything is launched, the entry's name first in the text.  Zero rows launch nothing (osn_interp_bwd
 * and osn_segment_reduce still write their whole output).
 *
 * osn_field_map: coords4f float32 [m, 4] rows (batch, x, y, z) in lattice units, any positions; the table is the stride's
 * (osn_coords_unique).  Per axis q = p / float(stride), f = floorf(q), base = int(f) * stride, t = q - f, a[0] = 1 - t,
 * a[1] = t.  Corner k = dx + 2 dy + 4 dz (the offset order of osn_kmap_build for ksize 2, x fastest) sits at
 * base + stride * (dx, dy, dz) in the row's batch: nbr[k, i] = its row in the table or -1, w[k, i] = (ax[dx] * ay[dy]) * az[dz],
 * both k-major [8, m].  A row with a non-finite coordinate, a batch outside [0, 65535) or a base with base or base + stride
 * outside (-32767, 32767) is invalid: eight -1, eight +0, and `bad` (int32, device, zeroed by the caller) is incremented with
 * an integer atomic.  The range test comes before the key is packed, so an invalid row never aliases a packed key.
 * osn_interp_fwd: y[i] = sum over the present k (nbr[k, i] in [0, n_in)), ascending, from +0, of w[k, i] * x[nbr[k, i]]; no
 * renormalisation over absent corners, a present corner of weight 0 is still multiplied (0 * inf = NaN stays).
 * osn_interp_bwd: `pair` int32 [n_pair] holds the indices e = k * m + i of the present corners sorted by (nbr[e], e), `offsets`
 * int64 [n_in + 1] the range of every voxel row in it:  gx[v] = sum over the row's pairs, in list order, from +0, of
 * w[e] * gy[e % m].  Every element of gx is written; an entry outside [0, 8 m) is skipped.
 * osn_segment_reduce: y[u] = the rows order[offsets[u] .. offsets[u + 1]) of x (order int32 [n], offsets int64 [n_seg + 1]) added
 * one by one in list order from +0; OSN_SEGMENT_AVG divides the sum once by float(length) (IEEE; an empty segment gives 0).  One
 * thread per segment and column group walks the list: a segment of hundreds of rows is correct and slow.                      */
#define OSN_SEGMENT_SUM 0
#define OSN_SEGMENT_AVG 1
int osn_field_map(const uint64_t* table_keys, const int32_t* table_vals, int64_t cap, const float* coords4f, int64_t m, int stride,
                  int32_t* nbr, float* w, int32_t* bad, osn_stream_t stream);
int osn_interp_fwd(const float* x, int64_t n_in, const int32_t* nbr, const float* w, int64_t m, int c, float* y, osn_stream_t stream);
int osn_interp_bwd(const float* gy, int64_t m, int c, const int32_t* pair, int64_t n_pair, const int64_t* offsets, const float* w,
                   int64_t n_in, float* gx, osn_stream_t stream);
int osn_segment_reduce(const float* x, int64_t n, int c, const int32_t* order, const int64_t* offsets, int64_t n_seg, int mode, float* y,
                       osn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENSCENE_AMD_H */
