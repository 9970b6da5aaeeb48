/* dcdf_k2r.h -- C ABI of the MI355X-native Heuristic K^2-Raster chunk engine.
 *
 * Drop-in boundary for ONE path of Arbol-Project/dcdf v0.2.0: `Chunk::build` and the
 * chunk-level queries.  Every entry point names the reference interface it replaces
 * (file:line relative to /root/reference/dcdf/src/).  A Rust `dcdf` fork binds these
 * with a plain `extern "C"` block; nothing here mentions torch.
 *
 * All encoded byte strings are bit-identical to the reference's `Chunk::write_to`
 * (chunk.rs:235-243).  Panics of the reference are negative return codes here.
 * The library needs a gfx950 GPU: every compute entry point returns
 * DCDF_ERR_NO_DEVICE when none is present -- there is no CPU fallback.
 */
#ifndef DCDF_K2R_H
#define DCDF_K2R_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* MMEncoding byte codes, mmstruct.rs:36-43 */
enum { DCDF_I32 = 4, DCDF_I64 = 8, DCDF_F32 = 32, DCDF_F64 = 64 };

/* memory space of caller-owned buffers */
enum { DCDF_MEM_HOST = 0, DCDF_MEM_DEVICE = 1 };

/* return / status codes (0 = ok) */
enum {
    DCDF_OK = 0,
    DCDF_ERR_BAD_ARG = -1,       /* instants == 0, bad dtype, null pointer ...                     */
    DCDF_ERR_NONFINITE = -2,     /* to_fixed on +-inf                       fixed.rs:39-41         */
    DCDF_ERR_PRECISION = -3,     /* to_fixed precision loss, round=false    fixed.rs:47-59         */
    DCDF_ERR_OVERFLOW = -4,      /* fixed-point value does not fit i64      fixed.rs:65-70         */
    DCDF_ERR_BOUNDS = -5,        /* query outside the chunk                 mmarray.rs:218-229     */
    DCDF_ERR_TOO_MANY_LOGS = -6, /* unreachable through build (254 cap)     block.rs:27-32         */
    DCDF_ERR_FORMAT = -7,        /* malformed encoded chunk on open         chunk.rs:247-266       */
    DCDF_ERR_UNSUPPORTED = -8,   /* sidelen > 1024 (fused kernel: k = 2, sidelen 16..256) */
    DCDF_ERR_NO_DEVICE = -9,     /* no gfx950 device / HIP runtime failure                         */
    DCDF_ERR_NOMEM = -10,
    DCDF_ERR_CAPACITY = -11,     /* result buffer too small (search): *n holds the needed count    */
    DCDF_ERR_INTERNAL = -12,     /* an internal consistency guard of the kernels tripped (a bug)     */
    DCDF_ERR_HIP = -13,          /* a HIP runtime call failed (launch failure, fault ...): dcdf_last_hip_error() */
    DCDF_ERR_HIP_INVALID = -14   /* HIP rejected an argument (bad device pointer / value)                        */
};

/* One `Chunk::build` input: a borrowed strided 3-D view [instants, rows, cols]
 * (mmbuffer.rs:255-260; tile slices are non-contiguous, mmbuffer.rs:517-522).
 * Not mutated, no pointer retained after the call returns. */
typedef struct dcdf_tile_desc {
    const void* base;                      /* element [0,0,0]                                   */
    int32_t dtype;                         /* DCDF_I32 / I64 / F32 / F64                         */
    int32_t _pad0;
    int64_t stride_t, stride_r, stride_c;  /* in ELEMENTS                                        */
    uint32_t instants, rows, cols;
    uint8_t fractional_bits;               /* floats only (mmbuffer.rs:554-571)                  */
    uint8_t round;                         /* floats only: lossy rounding allowed (fixed.rs:46)  */
    uint8_t _pad1[2];
} dcdf_tile_desc;

/* One `MMStruct3Build` (mmstruct.rs:24-34) for a Subchunk: serialized bytes + counters. */
typedef struct dcdf_encoded {
    uint8_t* bytes;       /* == Chunk::write_to image (chunk.rs:235-243); library-owned host memory   */
    size_t len;           /* == Chunk::size()  (chunk.rs:272-277)                                      */
    uint32_t snapshots;   /* chunk.rs:93-94                                                            */
    uint32_t logs;
    int32_t status;       /* per-tile DCDF_* code; bytes == NULL when != 0                             */
    int32_t kernel;       /* dcdf_encoder_tile_kernel of the tile as the batch staged it (host tiles are packed dense): */
                          /* 1 << 24 | loader << 16 | padded << 8 | log2_sidelen, or the universal kernel's key          */
                          /* (< 1 << 24); 0 for a rejected tile.  (Was padding, always 0: same layout, ABI 3.)           */
    int64_t* minmax;      /* [instants][2] stored-value (min,max) per instant = root of each k2 tree;  */
                          /* what Superchunk::build recomputes at superchunk.rs:144 (mmbuffer.rs:366)  */
} dcdf_encoded;

/* ---- encode -------------------------------------------------------------------------------- */

/* Replaces `Chunk::build(buffer, shape, k)` (chunk.rs:42-96) called per tile from
 * superchunk.rs:169, for n independent tiles at once.  Returns 0 if the call itself ran
 * (inspect out[i].status per tile) or a negative code for a whole-call failure.
 * `mem` says where tiles[i].base lives.  *out is an array of n records; free with
 * dcdf_free_encoded(*out, n). */
int dcdf_chunk_build_batch(const dcdf_tile_desc* tiles, size_t n, int k, int mem, dcdf_encoded** out);

/* Single tile == batch of 1 (chunk.rs:42). */
int dcdf_chunk_build(const dcdf_tile_desc* tile, int k, int mem, dcdf_encoded** out);

void dcdf_free_encoded(dcdf_encoded* out, size_t n);

/* Device-resident encode session (what bench.py times: inputs already in HBM, outputs stay in HBM).
 * tiles[i].base must be device pointers.  `out_cap_per_tile` bytes of device output are reserved
 * per tile (0 = library default = raw tile bytes + 4 KiB). */
typedef struct dcdf_encoder dcdf_encoder;
int dcdf_encoder_create(const dcdf_tile_desc* tiles, size_t n, int k, size_t out_cap_per_tile, dcdf_encoder** enc);
/* Which kernel dcdf_encoder_create chose for tile i, from the session's own tables (what the tests assert instead of restating
 * the rule).  A fused-kernel tile: *log2_sidelen = 4..8, *padded = 0 / 1 (rows or cols below the sidelen), *loader = 0 (the
 * generic strided loader) or 1..4 (the 16-byte row loader of int32 / float32 / int64 / float64 tiles: dense rows, 16-byte
 * aligned base, row and instant strides), *generic_key = 0.  A tile of the universal kernel: *generic_key = k << 8 | levels, the
 * other three -1.  Any out pointer may be NULL.  Returns the tile's validation code (then nothing is written) when create
 * rejected it.  A fused tile whose values turn out beyond the fused kernel's 2^30 contract is re-encoded by the universal
 * kernel at run time; this still reports the fused class it was queued for. */
int dcdf_encoder_tile_kernel(const dcdf_encoder* enc, size_t i, int32_t* log2_sidelen, int32_t* padded, int32_t* loader,
                             uint32_t* generic_key);
/* Launches the encode kernels on the session's stream and waits.  kernel_ms (may be NULL) receives
 * the HIP-event time of the encode kernel alone. */
int dcdf_encoder_run(dcdf_encoder* enc, float* kernel_ms);
/* Per-tile results of the last run (host copies of the small tables; bytes stay on the device). */
int dcdf_encoder_result(dcdf_encoder* enc, size_t i, int32_t* status, uint64_t* len, uint32_t* snapshots,
                        uint32_t* logs, const uint8_t** device_bytes);
/* Copies tile i's encoded bytes to host memory `dst` (cap >= len). */
int dcdf_encoder_fetch(dcdf_encoder* enc, size_t i, uint8_t* dst, size_t cap);
/* Sum of len over tiles with status 0 (for the algorithmic-bytes figure). */
uint64_t dcdf_encoder_total_bytes(dcdf_encoder* enc);
/* The final host-side gather of one GPU's encoded buffers (superchunk.rs:183-235 consumes them in tile order): tile i's
 * bytes land at dst + offsets[i] (16-byte aligned starts, lens[i] bytes; 0 for failed tiles), packed on the device and
 * copied back in one transfer; minmax (may be NULL) receives the per-(tile, instant) stored (min,max) pairs in tile
 * order, 2 * instants words per tile (what Superchunk::build recomputes at superchunk.rs:144).
 * dcdf_encoder_gather_size tells how large dst (bytes) and minmax (int64 words) must be. */
int dcdf_encoder_gather_size(dcdf_encoder* enc, uint64_t* packed_bytes, uint64_t* minmax_words);
int dcdf_encoder_gather(dcdf_encoder* enc, uint8_t* dst, size_t cap, uint64_t* offsets, uint64_t* lens, int64_t* minmax);
/* Content addressing of the stored chunk objects, computed where the encoded bytes lie (HBM): digests[32*i ..] =
 * SHA-256 of the object the reference would store for tile i -- u16 0xDCE0, u32 1, NODE_MMSTRUCT3 (2),
 * NODE_SUBCHUNK (4), big-endian, then the Chunk::write_to bytes (resolver.rs:17-18,126-138; mmstruct.rs:215-218) --
 * i.e. the digest inside its CID: CIDv1, codec 0x12, multihash sha2-256 (testing.rs:172-183).  Zeros for tiles that
 * failed.  `digests` is host memory; call after dcdf_encoder_run. */
int dcdf_encoder_object_sha256(dcdf_encoder* enc, uint8_t* digests, float* kernel_ms);
void dcdf_encoder_destroy(dcdf_encoder* enc);

/* ---- superchunk assembly (the caller of Chunk::build) ---------------------------------------- */

/* One object the reference would hand to `resolver.save` (resolver.rs:126-138): the 7-byte header (u16 0xDCE0, u32 1,
 * u8 node type) + the node, and its CID as MemoryMapper names it (testing.rs:172-183: CIDv1, codec 0x12, sha2-256). */
typedef struct dcdf_stored_object {
    uint8_t cid[36];
    uint8_t* bytes;
    size_t len;
} dcdf_stored_object;

/* `MMStruct3Build` of a Superchunk (mmstruct.rs:24-34) plus the objects to store: framed sub-chunks (mmstruct.rs:215-218),
 * nested Superchunk nodes, `Links` nodes (links.rs:65-76), de-duplicated by CID like `external_references`
 * (superchunk.rs:199-235), in save order; the LAST object is the Superchunk node itself (superchunk.rs:672-706), which
 * `Superchunk::build` leaves to its caller to save. */
typedef struct dcdf_superchunk {
    dcdf_stored_object* objects;
    size_t n_objects;
    uint64_t size;
    uint32_t elided, local, external, snapshots, logs;
} dcdf_superchunk;

/* Replaces `Superchunk::build(resolver, buffer, shape, levels, k)` (superchunk.rs:88-270): uniform-tile elision from
 * per-tile per-instant (min,max) computed on the device (mmbuffer.rs:366-499), per-tile fractional bits
 * (superchunk.rs:167), one batched Chunk::build launch per level, nested superchunks, the reference table, the
 * instant-major min / max Dacs, Links, object framing and CIDs.  `buffer` = the whole [instants, rows, cols] view
 * (fractional_bits / round as the caller's MMBuffer3 carries them); sum(levels) must equal ceil(log_k(max(rows, cols))). */
int dcdf_superchunk_build(const dcdf_tile_desc* buffer, const uint32_t* levels, size_t n_levels, int k, int mem,
                          dcdf_superchunk** out);
void dcdf_free_superchunk(dcdf_superchunk* s);

/* ---- query --------------------------------------------------------------------------------- */

typedef struct dcdf_chunk dcdf_chunk; /* an opened, device-resident encoded chunk */

/* geom::Cube (geom.rs:71-103): half-open bounds; reversed bounds are swapped as in the reference. */
typedef struct dcdf_cube {
    uint32_t start, end, top, bottom, left, right;
} dcdf_cube;

/* Replaces `Chunk::read_from` (chunk.rs:247-266) + upload.  `bytes` is host memory.  The stream is validated structurally
 * (DCDF_ERR_FORMAT otherwise) and copied to the device; for k = 2 chunks of sidelen 32..256 a 24-byte entry per 16 x 16
 * square and instant is built next to it on the device (where the query walks of that square start, and the square's value
 * range, which search prunes with). */
int dcdf_chunk_open(const uint8_t* bytes, size_t len, dcdf_chunk** h);
void dcdf_chunk_close(dcdf_chunk* h);
/* Chunk::shape (chunk.rs:119-123), encoding / fractional_bits (chunk.rs:33-38), block count. */
int dcdf_chunk_info(const dcdf_chunk* h, uint32_t shape[3], int32_t* encoding, uint32_t* fractional_bits,
                    uint32_t* n_blocks);

/* Byte offsets of the instants' Snapshots / Logs inside the chunk (off[instants + 1], the last = the chunk's length) and,
 * per instant, the instant of its block's snapshot (may be NULL): the encoded bytes a decode of instant i can touch are
 * [off[i], off[i + 1]) and the snapshot's range -- the decode path's algorithmic bytes. */
int dcdf_chunk_instant_layout(const dcdf_chunk* h, uint64_t* off, uint32_t* snapshot_of);

/* Replaces `Chunk::get` (chunk.rs:127-131): stored i64 value (fixed-point for float chunks). */
int dcdf_chunk_get(const dcdf_chunk* h, uint32_t instant, uint32_t row, uint32_t col, int64_t* out);
/* Replaces `Chunk::fill_cell` (chunk.rs:135-148): out[end-start] stored i64 values (host). */
int dcdf_chunk_fill_cell(const dcdf_chunk* h, uint32_t start, uint32_t end, uint32_t row, uint32_t col, int64_t* out);
/* Replaces `Chunk::fill_window` (chunk.rs:152-158) with MMBuffer3::set conversion (mmbuffer.rs:292-299,
 * 505,525,560,622): writes [end-start][bottom-top][right-left] into the caller's typed strided HOST array. */
int dcdf_chunk_fill_window(const dcdf_chunk* h, const dcdf_cube* cube, void* out, int32_t out_dtype, int64_t stride_t,
                           int64_t stride_r, int64_t stride_c);
/* Replaces `Chunk::iter_search` (chunk.rs:213-229, 336-383): (instant,row,col) triples, sorted.
 * cap = capacity of `out` in triples; *n = number found (DCDF_ERR_CAPACITY if > cap). */
int dcdf_chunk_search(const dcdf_chunk* h, const dcdf_cube* cube, int64_t lower, int64_t upper, uint32_t* out,
                      size_t cap, size_t* n);

/* Batched queries against many opened chunks (BASELINE config 5).  All arrays are host memory.
 * fill_window: query q writes its window, dense row-major i64 stored values, at out + out_offset[q]. */
int dcdf_query_fill_window_batch(dcdf_chunk* const* chunks, const dcdf_cube* cubes, size_t nq, int64_t* out,
                                 const uint64_t* out_offset, float* kernel_ms);
/* search: per-query counts in counts[q]; triples of query q at out + 3*offsets[q] (offsets = exclusive
 * prefix of counts, written by the call); cap in triples. */
int dcdf_query_search_batch(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const int64_t* lower,
                            const int64_t* upper, size_t nq, uint32_t* out, size_t cap, uint64_t* counts,
                            uint64_t* offsets, float* kernel_ms);

/* The same with a typed result and a result that may stay on the device: out_dtype = DCDF_I32 / I64 / F32 / F64 is the
 * element type written (MMBuffer3::set, mmbuffer.rs:292-299: integers as stored, floats through from_fixed, fixed.rs:81-86);
 * out_mem = DCDF_MEM_DEVICE: `out` is device memory, the decode kernel writes window q at out + out_offset[q] (ELEMENTS of
 * out_dtype) itself and nothing crosses PCIe.  An int32 result of int32 chunks moves half the bytes of the i64 form.  Every
 * arity and output type: a batch holding any k * k > 64 chunk is decoded cell by cell, typed the same way. */
int dcdf_query_fill_window_batch_typed(dcdf_chunk* const* chunks, const dcdf_cube* cubes, size_t nq, void* out,
                                       int32_t out_dtype, int out_mem, const uint64_t* out_offset, float* kernel_ms);
/* dcdf_query_search_batch whose triples may stay on the device (out_mem = DCDF_MEM_DEVICE: `out` is device memory of `cap`
 * triples); counts / offsets are always host arrays. */
int dcdf_query_search_batch_mem(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper,
                                size_t nq, uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets,
                                float* kernel_ms);
/* Many point / cell-series queries in ONE launch -- what Superchunk::get / fill_cell (superchunk.rs:313-400) and the
 * Span / Dataset layers above them route to their chunks.  points = n x {instant, row, col}; out[i] = the stored i64 value
 * of point i of chunks[i] (Chunk::get, chunk.rs:127-131).  cells = n x {start, end, row, col}; series i goes to
 * out + out_offset[i] (Chunk::fill_cell, chunk.rs:135-148).  out_mem as above. */
int dcdf_query_get_batch(dcdf_chunk* const* chunks, const uint32_t* points, size_t n, int64_t* out, int out_mem,
                         float* kernel_ms);
int dcdf_query_fill_cell_batch(dcdf_chunk* const* chunks, const uint32_t* cells, size_t n, int64_t* out,
                               const uint64_t* out_offset, int out_mem, float* kernel_ms);
/* Opens n chunks at once.  mem = DCDF_MEM_HOST: as n calls of dcdf_chunk_open.  mem = DCDF_MEM_DEVICE: bytes[i] are DEVICE
 * pointers, e.g. dcdf_encoder_result's `device_bytes` -- the streams are packed into one slab, parsed on the device (one
 * thread per chunk, bounds-checked) and the side-16 tables of all their instants are built by one launch; nothing is copied
 * to the host but the per-chunk metadata.  Device input gets dcdf_chunk_open's structural validation as well, on the device (a wave per
 * instant: popcounts against the Dac and eqB lengths, rank indexes).  status (may be NULL): one code per chunk;
 * out[i] = NULL where it is not 0.  Every handle is closed with dcdf_chunk_close; the slab goes with the last one. */
int dcdf_chunk_open_batch(const uint8_t* const* bytes, const uint64_t* lens, size_t n, int mem, dcdf_chunk** out,
                          int32_t* status);

/* ---- a whole raster of chunks: the routing of the layers above ------------------------------------------------------- */
/* A variable as dcdf lays it out: time segments of chunk_size instants (Variable::append, dataset.rs:838), each cut into
 * tile x tile sub-arrays (Superchunk::build, superchunk.rs:127-181); chunks[(segment * ntiles_r + ti) * ntiles_c + tj], every chunk
 * with the shape its place gives it.  The handle keeps the chunk table on the device.  Lifetime: the raster refers to the chunks'
 * device buffers; it shares the ownership of the slab of chunks opened by dcdf_chunk_open_batch (closing such a chunk first is
 * fine), chunks opened one by one (dcdf_chunk_open) must stay open until dcdf_raster_destroy. */
typedef struct dcdf_raster dcdf_raster;
int dcdf_raster_create(dcdf_chunk* const* chunks, size_t n_chunks, const uint32_t shape[3], uint32_t tile, uint32_t chunk_size,
                       dcdf_raster** out);
void dcdf_raster_destroy(dcdf_raster* r);
/* fill_window of nq dataset-level cubes (raster coordinates): each is split at segment / tile boundaries where Span::fill_window
 * (span.rs:190-216) and Superchunk::subchunks_for (superchunk.rs:589-633) split it, every piece is decoded by the same launch
 * straight into its place in the window; window q is dense [instants][rows][cols] of out_dtype at out + out_offset[q] (elements),
 * host or device memory.  k * k > 64 chunks: DCDF_ERR_UNSUPPORTED (use the per-chunk entry points). */
int dcdf_raster_fill_window_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype,
                                  int out_mem, const uint64_t* out_offset, float* kernel_ms);
/* Decompress: the cubes of a raster (plain or tiled), dense [instants][rows][cols] of out_dtype at out + out_offset[q]
 * (elements), host or device memory -- the same result, bit for bit, as dcdf_raster_fill_window_batch for the same
 * arguments.  Meant for whole tiles and long time ranges: every chunk leaf that has a side-16 table is decoded block by
 * block (one Snapshot visit per block and region); the others, and elided leaves, by the kernels fill_window uses.
 * stats (may be NULL): cells written by {bulk kernel, fallback walk, elided fill}. */
int dcdf_raster_decode_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, void* out, int32_t out_dtype,
                             int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* Reduce over time: per cell (row, col) of each cube, statistics over its instants of the values dcdf_raster_decode_batch returns
 * when out_dtype is the encoding of the leaf that holds the cell, widened to double: x[t] = (double)n for DCDF_I32 / I64 leaves,
 * (double)from_fixed in float for DCDF_F32 leaves, from_fixed in double for DCDF_F64 leaves, NaN for a stored 0 of a float leaf.
 *   DCDF_REDUCE_MIN / MAX   fmin / fmax over the non-NaN x[t]; NaN when there is none
 *   DCDF_REDUCE_SUM         s = 0.0; for t ascending: if x[t] is not NaN: s = s + x[t] -- sequential, in instant order, one IEEE
 *                           double addition per instant, so the result does not depend on how the work is cut
 *   DCDF_REDUCE_COUNT       the number of non-NaN x[t]
 *   DCDF_REDUCE_MEAN        SUM / COUNT (one IEEE division); NaN when COUNT is 0
 * Cube q writes popcount(ops) planes in ascending bit order, each dense [rows][cols] float64, from out + out_offset[q]
 * (elements), host or device memory; a cube of zero volume writes nothing.  stats (may be NULL): cells READ by {bulk kernel,
 * fallback walk, elided leaves}, the numbers dcdf_raster_decode_batch reports for the same cubes.  ops == 0 or a bit above 16:
 * DCDF_ERR_BAD_ARG; k * k > 64 chunks: DCDF_ERR_UNSUPPORTED. */
enum { DCDF_REDUCE_MIN = 1, DCDF_REDUCE_MAX = 2, DCDF_REDUCE_SUM = 4, DCDF_REDUCE_COUNT = 8, DCDF_REDUCE_MEAN = 16 };
int dcdf_raster_reduce_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, double* out, int out_mem,
                                  const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* Grouped reduce over time: dcdf_raster_reduce_time_batch's statistics, per cell, separately for every group of a per-instant
 * label array -- monthly means from daily data, a month-of-year climatology -- from ONE walk of each unit's instants.  Cubes, ops
 * (DCDF_REDUCE_*), out_mem, out_offset, stats and kernel_ms are exactly dcdf_raster_reduce_time_batch's: reversed bounds are
 * swapped, nq == 0 is fine, stats and kernel_ms may be NULL, stats are the numbers dcdf_raster_decode_batch reports for the same
 * cubes (the labels do not change them).
 *   labels   in HOST memory: instant i of cube q, counted from the cube's first instant after normalisation, has label
 *            labels[label_offset[q] + i] and belongs to group g when that equals g < n_groups; DCDF_GROUP_NONE and every other
 *            value >= n_groups belong to no group: such an instant contributes nowhere.  1 <= n_groups <= 65535, for all cubes.
 * With x[t] as above, per cell and group g over the instants of the group in ascending order: MIN / MAX = fmin / fmax over the
 * non-NaN x; SUM = the sequential chain s = 0.0, s = s + x[t]; COUNT = the number of non-NaN x; MEAN = SUM / COUNT (one
 * division).  A group without an instant, or whose x are all NaN, gets NaN, NaN, +0.0, 0, NaN.  Cube q writes popcount(ops) arrays
 * in ascending bit order from out + out_offset[q] (elements), each dense [n_groups][rows][cols] float64; every element of them is
 * written whatever the memory held, nothing outside them is; a cube without instants, rows or columns writes nothing.  The result
 * depends on no cut of the work: with n_groups == 1 and all labels 0 it is dcdf_raster_reduce_time_batch bit for bit, and for any
 * labels group g equals reduce_time of the sub-series of the instants labelled g.
 * DCDF_ERR_BAD_ARG: ops == 0 or a bit above 16, n_groups 0 or above 65535, NULL labels / label_offset / cubes / out / out_offset
 * with nq > 0, an unknown out_mem; DCDF_ERR_BOUNDS: a cube outside the raster; DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
#define DCDF_GROUP_NONE 0xffffu
int dcdf_raster_reduce_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint16_t* labels,
                                         const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem,
                                         const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* Moments over time: per cell (row, col) of each cube, how many values it has, their mean, variance and standard deviation --
 * what a standardised anomaly (x - mean) / std or a variability map needs, mean and std from ONE walk.  Cubes, out_mem,
 * out_offset, stats and kernel_ms are exactly dcdf_raster_reduce_time_batch's; labels, label_offset, n_groups and
 * DCDF_GROUP_NONE exactly dcdf_raster_reduce_time_groups_batch's.  ops is a non-empty set of DCDF_MOMENT_*, ddof (the divisor of
 * VAR is COUNT - ddof) 0 or 1.
 * With x[t] as above, the state of a cell -- per group, in the grouped call -- is four doubles (c, K, s1, s2), at first
 * (0, NaN, +0.0, +0.0).  For t ascending every non-NaN x[t] does
 *     if (c == 0) K = x;   d = x - K;   s1 = s1 + d;   s2 = s2 + d * d;   c = c + 1;
 * each one IEEE double operation (the product rounded, then the sum: nothing is contracted into an fma), sequentially in
 * instant order as DCDF_REDUCE_SUM's chain is, so the result depends on no cut of the work.  Then, per cell (and group):
 *     COUNT = c;   m = s1 / c;   MEAN = K + m;   q = s2 - s1 * m, +0.0 where that is negative;
 *     VAR = q / (c - ddof) when c > ddof, else NaN;   STD = sqrt(VAR), correctly rounded.
 * K, the shift, is the series' first value, a sample of the series: (mean - K)^2 / VAR <= n, which bounds the relative error of
 * VAR by the order of (n + 2)^2 * 2^-53.  Consequences: a constant series has VAR exactly +0.0 and MEAN
 * exactly its value; one value with ddof = 1 gives VAR = STD = NaN; MEAN is K + s1 / c, not SUM / COUNT -- it may differ from
 * DCDF_REDUCE_MEAN in the last bits and is offered so that mean and std come from one walk --; for integer leaves with
 * |x| < 2^53 a constant added to every value leaves VAR and STD unchanged bit for bit, because every d is exact.
 * Cube q writes popcount(ops) planes in the order COUNT, MEAN, VAR, STD from out + out_offset[q] (elements), each dense
 * [rows][cols] float64 -- in the grouped call [n_groups][rows][cols], group g the moments of the instants labelled g in order (its
 * K is the group's first value).  A cell or group without a value gets 0, NaN, NaN, NaN.  Every element of the planes is written,
 * nothing outside them is; a cube without instants, rows or columns writes nothing.  The grouped call with n_groups == 1 and all
 * labels 0 is the plain call bit for bit.
 * DCDF_ERR_BAD_ARG: ops == 0 or a bit above 8, ddof > 1, (grouped) n_groups 0 or above 65535 and NULL labels / label_offset with
 * nq > 0, NULL r / cubes / out / out_offset, an unknown out_mem (nq == 0 is fine, stats and kernel_ms may be NULL);
 * DCDF_ERR_BOUNDS: a cube outside the raster; DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
enum { DCDF_MOMENT_COUNT = 1, DCDF_MOMENT_MEAN = 2, DCDF_MOMENT_VAR = 4, DCDF_MOMENT_STD = 8 };
int dcdf_raster_moments_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof, double* out, int out_mem,
                                   const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
int dcdf_raster_moments_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t ddof,
                                          const uint16_t* labels, const uint64_t* label_offset, uint32_t n_groups, double* out, int out_mem,
                                          const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* The step and the finish above on the host -- no GPU call, the functions the kernels run.  Continues state = (c, K, s1, s2)
 * over x[0 .. n) in order, NaN skipped, and leaves the new state there; when out is not NULL, finishes that state into out =
 * (COUNT, MEAN, VAR, STD) with ddof.  A series starts from (0, NaN, 0, 0).  DCDF_ERR_BAD_ARG: NULL state, NULL x with n > 0,
 * ddof > 1. */
int dcdf_moments_host(const double* x, size_t n, uint32_t ddof, double state[4], double out[4]);
/* Regression over time, the contract and its host form: the least-squares line of a series x[i] against a per-instant regressor
 * e[i] -- a trend when the regressor is the instant index, a regression / correlation against an index series otherwise.  The
 * raster calls below run it per cell of a cube, x[i] being reduce_time's x[t].
 * The state is seven doubles (c, K, sy, syy, se, see, sey), at first (0, NaN, +0.0, +0.0, +0.0, +0.0, +0.0).  For i ascending every
 * pair with a non-NaN x[i] does
 *     if (c == 0) K = x;  d = x - K;
 *     sy = sy + d;  syy = syy + d * d;  se = se + e;  see = see + e * e;  sey = sey + e * d;  c = c + 1
 * -- each one IEEE double operation, nothing contracted into an fma; a NaN x changes nothing.
 * Finishing: n = c, me = se / n, my = sy / n, See = max(see - se * me, +0.0), Syy = max(syy - sy * my, +0.0), Sey = sey - se * my;
 *     COUNT = c;  SLOPE = Sey / See when c >= 2 and See > 0, else NaN;  INTERCEPT = (K + my) - SLOPE * me, NaN when SLOPE is;
 *     CORR = Sey / sqrt(See * Syy), the root correctly rounded, clamped to [-1, 1], when additionally Syy > 0, else NaN.
 * Every NaN is the one quiet NaN.  The state is continued whole, so the result depends on no cut of the series.  A constant series
 * has SLOPE exactly +0.0, INTERCEPT its value and CORR NaN; one valid pair gives NaN but for COUNT; for integer values with
 * |x| < 2^53 a constant added to every value changes no bit of SLOPE or CORR, because every d is exact.
 * THE REGRESSOR ENTERS AS GIVEN: nothing shifts it, and INTERCEPT is the fitted value at e = 0.  The values are shifted by K, the
 * regressor is not, so accuracy needs a regressor near zero -- |e| of the order of its own spread.  With a the least |e| among the
 * n valid pairs and rho = a / sqrt(See), the error of SLOPE * sqrt(See / Syy) and of CORR stays below
 * 6 (1 + rho)^2 (n + 2)^2 2^-53 (derived in DESIGN.md section 4n): 6 (n + 2)^2 2^-53 when 0 is among those values (a first
 * value of 0 whose x is no NaN; 0.22 n^2 2^-53 was the worst seen); with the instant index offset by 20000 the error was
 * 3.7e3 n^2 2^-53 already at n = 3.  A caller whose regressor is far from zero (years, time stamps) passes e[i] - e[0] and reads
 * INTERCEPT as the fitted value at the first instant. */
enum { DCDF_REGRESS_COUNT = 1, DCDF_REGRESS_SLOPE = 2, DCDF_REGRESS_INTERCEPT = 4, DCDF_REGRESS_CORR = 8 };
/* The step and the finish above on the host -- no GPU call.  Continues state = (c, K, sy, syy, se, see, sey) over the pairs
 * (x[i], e[i]), i in [0, n) in order, NaN x skipped, and leaves the new state there; when out is not NULL, finishes that state into
 * out = (COUNT, SLOPE, INTERCEPT, CORR).  A series starts from (0, NaN, 0, 0, 0, 0, 0).
 * DCDF_ERR_BAD_ARG: NULL state, NULL x or e with n > 0, a value of e that is not finite (the state is then untouched). */
int dcdf_regress_host(const double* x, const double* e, size_t n, double state[7], double out[4]);
/* The regression above per cell (row, col) of each cube -- a trend map, the correlation of every cell with an index series --, whole
 * or, in the grouped call, separately for every group of a per-instant label array.  The cube is decoded band by band into the
 * bounded device slab of dcdf_raster_quantile_time_batch and every cell's series is read from there once; the cube never reaches
 * the host.  The calls take plain and tiled rasters, elided leaves included.  Cubes, out_mem, out_offset, stats and kernel_ms are
 * exactly dcdf_raster_reduce_time_batch's; labels, label_offset, n_groups and DCDF_GROUP_NONE exactly
 * dcdf_raster_reduce_time_groups_batch's.  ops is a non-empty set of DCDF_REGRESS_*.
 *   regressor   in HOST memory: instant i of cube q, counted from the cube's first instant after normalisation, has the regressor
 *               value regressor[regressor_offset[q] + i] (offsets in elements, as label_offset); it enters as given (above).  NULL,
 *               together with a NULL regressor_offset: the instant index i itself, 0, 1, 2, ... as doubles.  A value that is not
 *               finite anywhere in the array of a cube that has cells is DCDF_ERR_BAD_ARG before anything is launched.
 * Per cell -- and group g, over the instants labelled g in ascending order, each with its own regressor value -- the pairs
 * (x[t], e[t]) go through the step above from the initial state, then the finish.  Cube q writes popcount(ops) planes in the order
 * COUNT, SLOPE, INTERCEPT, CORR from out + out_offset[q] (elements), each dense [rows][cols] float64 -- in the grouped call
 * [n_groups][rows][cols].  A cell or group without a value gets 0, NaN, NaN, NaN.  Every element of the planes is written exactly
 * once, nothing outside them is; a cube without instants, rows or columns writes nothing.  The grouped call with n_groups == 1 and
 * all labels 0 is the plain call bit for bit, and the result depends on no cut of the work (K2R_QUANTILE_SLAB_BYTES, the slab's cap,
 * changes no bit).
 * DCDF_ERR_BAD_ARG: ops == 0 or a bit above 8, one of regressor / regressor_offset NULL and the other not, a regressor value that
 * is not finite, (grouped) n_groups 0 or above 65535 and NULL labels / label_offset with nq > 0, NULL r / cubes / out / out_offset,
 * an unknown out_mem (nq == 0 is fine, stats and kernel_ms may be NULL); DCDF_ERR_BOUNDS: a cube outside the raster;
 * DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
int dcdf_raster_regress_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const double* regressor,
                                   const uint64_t* regressor_offset, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                                   float* kernel_ms);
int dcdf_raster_regress_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const double* regressor,
                                          const uint64_t* regressor_offset, const uint16_t* labels, const uint64_t* label_offset,
                                          uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                                          float* kernel_ms);
/* Rolling windows over time: per cell (row, col) of each cube, the greatest and least sum (or mean) of every `window` consecutive
 * instants, when they occurred and how many windows counted -- the greatest 5-day total of a year (Rx5day), the wettest or driest
 * 30-day period and when it began, the lowest 7-day mean flow --, whole or, in the grouped call, for every group of a per-instant
 * label array.  The cube is decoded band by band into the bounded device slab of dcdf_raster_quantile_time_batch and every cell's
 * series is read from there; the cube never reaches the host.  The calls take plain and tiled rasters, elided leaves included.
 * Cubes, out_mem, out_offset, stats and kernel_ms are exactly dcdf_raster_reduce_time_batch's; labels, label_offset, n_groups and
 * DCDF_GROUP_NONE exactly dcdf_raster_reduce_time_groups_batch's.  DESIGN.md section 4o.
 *   values      x[i] is reduce_time's x[t] (reduce_widen of the stored integer with its own segment's encoding and fractional
 *               bits), instants i = 0 .. nt - 1 counted from the cube's first instant after normalisation.
 *   window      w, 1 .. 65535.  The window that ENDS at instant i covers [i - w + 1, i] and exists only for i >= w - 1: the cube's
 *               first w - 1 instants end no window (a caller who wants windows that reach back before `start` passes an earlier
 *               start).  c_i is the number of non-NaN values in it, S_i their EXACT real sum; NaN values contribute nothing.
 *   min_count   1 .. w: the window is valid iff c_i >= min_count.
 *   kind        DCDF_ROLLING_SUM or DCDF_ROLLING_MEAN.  MEAN requires min_count == window: a mean over a varying count is not an
 *               order on the sums.
 *   ops         a non-empty set of DCDF_ROLLING_*; cube q writes popcount(ops) planes in the order MAX, ARGMAX, MIN, ARGMIN, COUNT
 *               from out + out_offset[q] (elements), each dense [rows][cols] float64 -- in the grouped call [n_groups][rows][cols],
 *               the layout (statistics, groups, rows, cols) of dcdf_raster_moments_time_groups_batch.
 * MAX / MIN: the greatest / least S_i over the valid windows, rounded ONCE to the nearest double, ties to even; a sum of 0 is +0.0.
 * For MEAN that double is divided by (double)w, one IEEE division.  ARGMAX / ARGMIN: the LEAST i -- the window's last instant --
 * whose exact S_i is the greatest / least: the comparison is on the exact sums (192-bit integers at the 2^-63 scale), not on the
 * rounded doubles, so two sums that round to the same double but differ are not a tie.  COUNT: the number of valid windows.  With
 * no valid window (window > nt included): the one quiet NaN in the four others, +0.0 in COUNT.
 * Groups: a window belongs to the group of its LAST instant, labels[label_offset[q] + i], and reaches back over instants of any
 * label or none -- the Rx5day of a year may begin in the previous December.  Group g is the fold over the valid windows with label
 * g; ARGMAX / ARGMIN are still counted from the cube's first instant.  n_groups == 1 with all labels 0 is the plain call bit for
 * bit.
 * Every element of the planes is written exactly once, nothing outside them is; a cube without instants, rows or columns writes
 * nothing.  The sums are integers, so sliding a window and summing it again give the same bits: the result depends on no cut of
 * the work (K2R_QUANTILE_SLAB_BYTES, the slab's cap, changes no bit).  Consequences: window == 1 with SUM gives reduce_time's MAX,
 * MIN and COUNT bit for bit; a constant cell has ARGMAX == ARGMIN == w - 1.
 * Known cost: a group's windows are walked in ascending order, a run of consecutive instants sliding, every other window summed
 * again from its w values -- a labelling such as i % 7 reads O(w) values per window.
 * DCDF_ERR_BAD_ARG: ops == 0 or a bit above 16, window outside 1 .. 65535, min_count outside 1 .. window, a kind other than the
 * two, MEAN with min_count != window, (grouped) n_groups 0 or above 65535 and NULL labels / label_offset with nq > 0, NULL r /
 * cubes / out / out_offset, an unknown out_mem (nq == 0 is fine, stats and kernel_ms may be NULL); DCDF_ERR_BOUNDS: a cube outside
 * the raster; DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
enum { DCDF_ROLLING_MAX = 1, DCDF_ROLLING_ARGMAX = 2, DCDF_ROLLING_MIN = 4, DCDF_ROLLING_ARGMIN = 8, DCDF_ROLLING_COUNT = 16 };
enum { DCDF_ROLLING_SUM = 0, DCDF_ROLLING_MEAN = 1 };
int dcdf_raster_rolling_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window,
                                   uint32_t min_count, int32_t kind, double* out, int out_mem, const uint64_t* out_offset,
                                   uint64_t stats[3], float* kernel_ms);
int dcdf_raster_rolling_time_groups_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, uint32_t window,
                                          uint32_t min_count, int32_t kind, const uint16_t* labels, const uint64_t* label_offset,
                                          uint32_t n_groups, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3],
                                          float* kernel_ms);
/* Spell statistics over time: per cell (row, col) of each cube, on how many of its instants the value lay inside a range, and how
 * long and when the longest unbroken run of such instants was.  The call takes plain and tiled rasters, elided leaves included.
 * Cubes, out_mem, out_offset, stats and kernel_ms are exactly dcdf_raster_reduce_time_batch's: reversed bounds of a cube are
 * swapped, stats are the numbers dcdf_raster_decode_batch reports for the same cubes, a cube of zero volume writes nothing,
 * nq == 0 is fine, stats and kernel_ms may be NULL.  lower[q] / upper[q] are cube q's own bounds, in HOST memory: reversed bounds
 * are swapped, +-inf is unbounded, a NaN bound is DCDF_ERR_BAD_ARG.
 *   hit     instant i of a cell -- i counts from the cube's first instant, after normalisation -- is a hit iff the cell's stored
 *           integer lies in the set dcdf_value_bounds returns for the encoding and fractional bits of the leaf that holds the
 *           cell: [lo, hi], less 0 when skip_zero.  It is value search's rule and nothing else: a float leaf's NaN never hits, an
 *           integer leaf compares n itself with [ceil(lower), floor(upper)] (never rounded to double), a hit is exactly a cell
 *           dcdf_raster_search_values_batch reports for the same bounds, and an elided leaf uses its per-instant value with the
 *           eliding node's encoding and bits.
 * Per cell, over i ascending, with cur = the length of the run of hits that ends at i:
 *   DCDF_SPELL_COUNT          the number of hits
 *   DCDF_SPELL_LONGEST        the largest cur reached; 0 when there is no hit
 *   DCDF_SPELL_LONGEST_START  the i at which the first run of that length began (the state changes only when cur > longest: on
 *                             ties the earliest run wins); DCDF_SPELL_NONE when there is no hit
 *   DCDF_SPELL_FIRST / LAST   the first / last i that hit; DCDF_SPELL_NONE when there is none
 * Cube q writes popcount(ops) planes in ascending bit order, each dense [rows][cols] uint32, from out + out_offset[q] (elements),
 * host or device memory; nothing outside a cube's planes is written.  All of it is one sequential integer fold per cell whose
 * state every piece of the work hands on, so the result depends on no cut of the work.
 * DCDF_ERR_BAD_ARG: ops == 0 or a bit above 16; a NaN bound; NULL r, cubes, lower, upper, out or out_offset with nq > 0; an
 * unknown out_mem.  DCDF_ERR_BOUNDS: a cube outside the raster.  DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
enum { DCDF_SPELL_COUNT = 1, DCDF_SPELL_LONGEST = 2, DCDF_SPELL_LONGEST_START = 4, DCDF_SPELL_FIRST = 8, DCDF_SPELL_LAST = 16 };
#define DCDF_SPELL_NONE 0xffffffffu
int dcdf_raster_spells_batch(const dcdf_raster* r, const dcdf_cube* cubes, const double* lower, const double* upper, size_t nq,
                             uint32_t ops, uint32_t* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* Quantiles over time: per cell (row, col) of each cube, order statistics of its series -- the median, the 5th or 95th percentile
 * -- exact, selected on the device from a bounded slab of decoded values; the cube never reaches the host.  The call takes plain
 * and tiled rasters, elided leaves included.  Cubes, out_mem, out_offset, stats and kernel_ms are exactly
 * dcdf_raster_reduce_time_batch's: reversed bounds of a cube are swapped, stats are the numbers dcdf_raster_decode_batch reports
 * for the same cubes, a cube of zero volume writes nothing, nq == 0 is fine, stats and kernel_ms may be NULL.
 *   probs    n_probs doubles in HOST memory, shared by all cubes; 1 <= n_probs <= 16, each in [0, 1].
 *   x[t]     of a cell: reduce_time's x[t], the stored integer widened with the encoding and fractional bits of the leaf that holds
 *            the cell at that instant.  v[0 .. n) = the non-NaN x[t] in ascending order, n their count; -0.0 sorts before +0.0.
 *   n == 0   gives NaN.  Else h = (double)(n - 1) * p (one IEEE multiplication), j = floor(h), g = h - j, j1 = min(j + 1, n - 1):
 *   DCDF_QUANTILE_LOWER    v[j]
 *   DCDF_QUANTILE_HIGHER   v[j] when g == 0, else v[j1]
 *   DCDF_QUANTILE_NEAREST  v[j] when g < 0.5, v[j1] when g > 0.5; at g == 0.5 whichever of j, j1 is even
 *   DCDF_QUANTILE_LINEAR   v[j] when g == 0, else v[j] + (v[j1] - v[j]) * g: three separate IEEE double operations, no fused
 *                          multiply-add
 * p = 0 and p = 1 are DCDF_REDUCE_MIN and DCDF_REDUCE_MAX bit for bit, apart from the sign of a zero.  Cube q writes n_probs planes
 * in the order of probs, each dense [rows][cols] float64, from out + out_offset[q] (elements), host or device memory; nothing
 * outside a cube's planes is written.  The result is an order statistic of the cell's own values: it depends on no cut of the work.
 * DCDF_ERR_BAD_ARG: n_probs of 0 or above 16; a NaN or a value outside [0, 1] among probs; an unknown method; NULL r, cubes, probs,
 * out or out_offset; an unknown out_mem.  DCDF_ERR_BOUNDS: a cube outside the raster.  DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
enum { DCDF_QUANTILE_LOWER = 0, DCDF_QUANTILE_HIGHER = 1, DCDF_QUANTILE_NEAREST = 2, DCDF_QUANTILE_LINEAR = 3 };
int dcdf_raster_quantile_time_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const double* probs, uint32_t n_probs,
                                    int32_t method, double* out, int out_mem, const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* The selection dcdf_raster_quantile_time_batch runs per cell, as the device runs it, on the host: x is [instants][cells] doubles
 * (NaN = no value), out [n_probs][cells]; passes (may be NULL) [cells]: how many times the cell's series was read after the first.
 * Pure host function; no GPU, no HIP call (so it is testable on a CPU-only machine).  DCDF_ERR_BAD_ARG: a NULL pointer, the
 * probs / method errors above. */
int dcdf_quantile_select_host(const double* x, uint32_t instants, uint64_t cells, const double* probs, uint32_t n_probs, int32_t method,
                              double* out, uint32_t* passes);
/* Reduce over space: per instant of each cube, statistics over its SELECTED cells -- a series over an area.  The call takes
 * plain and tiled rasters.  Cube q is [start, end) x [top, bottom) x [left, right) (reversed bounds are swapped); its cell (r, c)
 * is selected when mask == NULL, or when the byte mask[mask_offset[q] + (r - top) * cols + (c - left)] is non-zero: a dense
 * row-major [rows][cols] mask of one byte per cell, host or device memory (mask_mem).  mask_offset == NULL only with mask == NULL.
 * x[r, c] of instant t is reduce_time's x[t]: the stored integer widened with the encoding and fractional bits of the leaf that
 * holds the cell ((double)n, from_fixed in float or in double, NaN for a stored 0 of a float leaf).  Over the selected cells:
 *   DCDF_REDUCE_MIN / MAX   fmin / fmax over the non-NaN x; NaN when there is none
 *   DCDF_REDUCE_COUNT       the number of non-NaN x
 *   DCDF_REDUCE_SUM         the EXACT real sum of the non-NaN x, rounded once to the nearest double, ties to even (what Python's
 *                           math.fsum returns); +0.0 when there is none.  It depends on no order and on no cut of the work:
 *                           every x is an integer multiple of 2^-63, and the sum is formed in integers.
 *   DCDF_REDUCE_MEAN        SUM / COUNT (one IEEE division); NaN when COUNT is 0
 * Cube q writes popcount(ops) series in ascending bit order, each dense [instants] float64, from out + out_offset[q] (elements),
 * host or device memory.  A cube without instants writes nothing; one with instants but no rows or columns, or with an all-zero
 * mask, writes the "none" values for every instant.  stats (may be NULL): cells read by {bulk kernel, fallback walk, elided
 * leaves}, the numbers dcdf_raster_decode_batch reports for the same cubes; the mask does not change them.  ops == 0 or a bit
 * above 16: DCDF_ERR_BAD_ARG; a cube outside the raster: DCDF_ERR_BOUNDS; k * k > 64 chunks: DCDF_ERR_UNSUPPORTED. */
int dcdf_raster_reduce_space_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint8_t* mask,
                                   const uint64_t* mask_offset, int mask_mem, double* out, int out_mem, const uint64_t* out_offset,
                                   uint64_t stats[3], float* kernel_ms);
/* The arithmetic DCDF_REDUCE_SUM of dcdf_raster_reduce_space_batch rests on, as the device runs it: n two's complement 128-bit
 * integers (hi[i], lo[i]), each shifted left by scale[i] & 255 (at most 63) and negated when scale[i] & 256, are added in 192
 * bits; *sum = that integer / 2^63 as the nearest double, ties to even.  Pure host function; no GPU, no HIP call (so it is
 * testable on a CPU-only machine).  DCDF_ERR_BAD_ARG: a NULL pointer, a scale beyond those bits. */
int dcdf_space_fold_records(const uint64_t* hi, const uint64_t* lo, const uint32_t* scale, size_t n, double* sum);
/* Zonal statistics: per instant of each cube, reduce_space's statistics for EVERY zone of a label raster at once -- one walk of
 * the encoded bytes, a [zones][instants] matrix per statistic.  The call takes plain and tiled rasters (elided leaves included).
 * Cubes, ops (DCDF_REDUCE_*), out_mem, stats and kernel_ms are exactly dcdf_raster_reduce_space_batch's: reversed bounds are
 * swapped, stats are the numbers dcdf_raster_decode_batch reports for the same cubes, nq == 0 is fine.
 *   labels   a dense row-major [rows][cols] array of uint16 per (normalised) cube; cube q's starts at element label_offset[q];
 *            host or device memory (label_mem).  Cell (r, c) belongs to zone labels[label_offset[q] + (r - top) * cols + (c - left)]
 *            when that value is < n_zones; DCDF_ZONE_NONE and every other value >= n_zones belong to no zone.  Nothing is
 *            validated per cell.  1 <= n_zones <= 65535, shared by all cubes.
 *   x        of a cell: reduce_space's x.  Per zone and instant, over the zone's cells:
 *   DCDF_REDUCE_MIN / MAX   fmin / fmax over the non-NaN x; NaN when there is none.  When both -0.0 and +0.0 occur in one zone
 *                           and instant, -0.0 is the minimum and +0.0 the maximum.
 *   DCDF_REDUCE_COUNT       the number of non-NaN x; 0 when there is none
 *   DCDF_REDUCE_SUM         the EXACT real sum of the non-NaN x, rounded once, ties to even (math.fsum); +0.0 when there is none
 *   DCDF_REDUCE_MEAN        SUM / COUNT (one IEEE division); NaN when COUNT is 0
 *            "None" covers a zone no cell carries, a zone whose cells are all NaN, and a cube without rows or columns.  Every
 *            piece of the work adds to integer accumulators, so the result depends on no order and on no cut of the work.
 * Cube q writes popcount(ops) matrices in ascending bit order, each dense [n_zones][instants] float64, from out + out_offset[q]
 * (elements), host or device memory.  A cube without instants writes nothing; nothing outside a cube's matrices is written.
 * DCDF_ERR_BAD_ARG: ops == 0 or a bit above 16; n_zones of 0 or above 65535; NULL labels, label_offset, cubes, out or out_offset
 * with nq > 0; an unknown *_mem.  DCDF_ERR_BOUNDS: a cube outside the raster.  DCDF_ERR_UNSUPPORTED: k * k > 64 chunks. */
#define DCDF_ZONE_NONE 0xffffu
int dcdf_raster_zonal_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, uint32_t ops, const uint16_t* labels,
                            const uint64_t* label_offset, int label_mem, uint32_t n_zones, double* out, int out_mem,
                            const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* The arithmetic DCDF_REDUCE_SUM of dcdf_raster_zonal_batch rests on, as the device runs it: a (zone, instant)'s sum at the 2^-63
 * scale is kept in six int64 counters, limb i weighing 2^(32 i); *sum = (the sum of limbs[i] * 2^(32 i)) / 2^63 as the nearest
 * double, ties to even, +0.0 for 0.  Pure host function; no GPU, no HIP call.  DCDF_ERR_BAD_ARG: a NULL pointer, a total that is
 * no 192-bit two's complement integer. */
int dcdf_zonal_fold_limbs(const int64_t limbs[6], double* sum);
/* Value histograms: per instant of each cube, how many of its SELECTED cells fall into every bin of shared edges -- the
 * distribution of values over an area.  The call takes plain and tiled rasters (elided leaves included).  Cubes, the mask
 * (mask, mask_offset, mask_mem) and stats are exactly dcdf_raster_reduce_space_batch's: reversed bounds are swapped, a non-zero
 * byte of the dense [rows][cols] mask of cube q selects the cell, stats are the numbers dcdf_raster_decode_batch reports for the
 * same cubes and the mask does not change them.
 *   edges   n_bins + 1 doubles in HOST memory, shared by all cubes, strictly increasing; -inf first and +inf last are allowed
 *           ("below" and "above" bins).  1 <= n_bins <= DCDF_HIST_MAX_BINS.
 *   x       of a cell: reduce_space's x, the stored integer n widened with the encoding and fractional bits of the leaf that holds
 *           the cell -- (double)(int32_t)n, (double)n, from_fixed in float widened to double, from_fixed in double, NaN for a stored
 *           0 of a float leaf.  NaN cells are counted nowhere.
 *   bin     a selected non-NaN cell is counted in bin b when edges[b] <= x < edges[b + 1]; the last bin takes edges[n_bins - 1]
 *           <= x <= edges[n_bins] (numpy.histogram's rule for explicit edges).  Cells below edges[0] or above edges[n_bins] are
 *           counted nowhere.
 * Cube q writes a dense [instants][n_bins] array of uint64 from out + out_offset[q] (elements), host or device memory.  A cube
 * without instants writes nothing; one with instants but no selected cell writes zeros; nothing outside a cube's array is
 * written.  With device memory the arrays themselves are the accumulators: the call zeroes them, then adds.  Counts are integers,
 * so the result depends on no order and on no cut of the work.
 * DCDF_ERR_BAD_ARG: NULL edges, out, out_offset or cubes; n_bins of 0 or above DCDF_HIST_MAX_BINS; a NaN edge; edges not strictly
 * increasing; a mask without offsets; an unknown *_mem.  DCDF_ERR_BOUNDS: a cube outside the raster.  DCDF_ERR_UNSUPPORTED:
 * k * k > 64 chunks.  nq == 0 is fine; stats and kernel_ms may be NULL. */
#define DCDF_HIST_MAX_BINS 256
int dcdf_raster_histogram_batch(const dcdf_raster* r, const dcdf_cube* cubes, size_t nq, const double* edges, uint32_t n_bins,
                                const uint8_t* mask, const uint64_t* mask_offset, int mask_mem, uint64_t* out, int out_mem,
                                const uint64_t* out_offset, uint64_t stats[3], float* kernel_ms);
/* The translation dcdf_raster_histogram_batch rests on: [lo[b], hi[b]] is the inclusive interval of the stored integers of a
 * chunk of this encoding and these fractional bits that bin b takes; lo[b] > hi[b] when it takes none.  x is monotone in the
 * stored integer, so the intervals are found by bisection with the decoder's own expression: (double)n rounds beyond 2^53 and
 * (float)(n - 1) beyond 2^24, so n < edge does not imply x < edge; with 62 fractional bits x decreases in n and the intervals
 * come out in reverse order.  Stored 0 of a float encoding (NaN) belongs to no bin: it is never an end of an interval, and where
 * it lies strictly inside one it is simply never counted.  Pure host function; no GPU, no HIP call (so it is testable on a
 * CPU-only machine).  DCDF_ERR_BAD_ARG: a NULL pointer, the edge errors above, an unknown encoding, float fractional_bits > 62. */
int dcdf_histogram_bounds(int32_t encoding, uint32_t fractional_bits, const double* edges, uint32_t n_bins, int64_t* lo, int64_t* hi);
/* search of nq dataset-level cubes: (instant, row, col) triples in RASTER coordinates (span.rs:231-270 adds the segment offset,
 * superchunk.rs:516-585 the tile origin); query q's triples are out[3 * offsets[q] .. + 3 * counts[q]), ordered by piece
 * (segment, tile row, tile col), sorted inside a piece. */
int dcdf_raster_search_batch(const dcdf_raster* r, const dcdf_cube* cubes, const int64_t* lower, const int64_t* upper, size_t nq,
                             uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets, float* kernel_ms);

/* ---- value search: real-valued bounds (what replaces the todo!() of MMArray3F32::search / MMArray3F64::search,
 * mmarray.rs:407-417 and 511-521: the bounds translated into each chunk's own fixed-point representation) ----------
 * A cell matches [lower, upper] iff the value the typed fill_window returns for it, v, satisfies lower <= v <= upper exactly:
 * DCDF_F32 / F64 chunks: v = from_fixed in float / double, (n - 1) / 2^(fractional_bits + 1) (fixed.rs:81-86; stored 0 is NaN
 * and never matches); DCDF_I32 / I64 chunks: v = n, i.e. n in [ceil(lower), floor(upper)].  Reversed bounds are swapped, +-inf
 * is unbounded, a NaN bound is DCDF_ERR_BAD_ARG.  Value search returns the cells' TRUE values on the instants where the integer
 * search reproduces the reference's quirk (log.rs:527-548).  The integer entry points above are unchanged. */

/* The matching stored integers of one chunk: [*lo, *hi], less 0 when *skip_zero (set only when *lo < 0 < *hi).  DCDF_OK and
 * *lo > *hi when nothing matches.  Pure host function; no GPU, no HIP call (so it is testable on a CPU-only machine).
 * DCDF_ERR_BAD_ARG: a NaN bound, an unknown encoding, float fractional_bits > 62 (beyond what Chunk::build accepts). */
int dcdf_value_bounds(int32_t encoding, uint32_t fractional_bits, double lower, double upper, int64_t* lo, int64_t* hi,
                      int32_t* skip_zero);
/* dcdf_chunk_search with real-valued bounds: sorted (instant,row,col) triples, cap / *n / DCDF_ERR_CAPACITY as there. */
int dcdf_chunk_search_values(const dcdf_chunk* h, const dcdf_cube* cube, double lower, double upper, uint32_t* out, size_t cap,
                             size_t* n);
/* dcdf_query_search_batch_mem with real-valued bounds (each query's bounds translated with its chunk's encoding and bits). */
int dcdf_query_search_values_batch(dcdf_chunk* const* chunks, const dcdf_cube* cubes, const double* lower, const double* upper,
                                   size_t nq, uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets,
                                   float* kernel_ms);
/* dcdf_raster_search_batch with real-valued bounds: k = 2 rasters translate them per piece on the device, with the piece's
 * chunk's encoding and fractional bits. */
int dcdf_raster_search_values_batch(const dcdf_raster* r, const dcdf_cube* cubes, const double* lower, const double* upper,
                                    size_t nq, uint32_t* out, size_t cap, int out_mem, uint64_t* counts, uint64_t* offsets,
                                    float* kernel_ms);

/* ---- rasters over stored Superchunks: elided tiles, nested levels, dataset-level get / fill_cell ----------------------------
 * A variable stored through Superchunk::build is a tree per time segment: a tile whose value is uniform at every instant is
 * elided (superchunk.rs:145-151; tiles outside the array too) and keeps one value per instant in its node's max Dac; a small
 * remainder tile may be one chunk at an upper level (superchunk.rs:153-163).  A tiled raster takes that tree flattened into its
 * leaves.  Leaves form the same grid as dcdf_raster_create's chunks: [(segment * nti + ti) * ntj + tj], leaf size `tile` =
 * k^(last k2_level), each with the shape its place gives it. */
typedef struct dcdf_raster_tile {
    dcdf_chunk* chunk;        /* NULL: elided leaf (Reference::Elided)                                                      */
    uint32_t row0, col0;      /* where the leaf starts inside `chunk` (non-zero only when one chunk spans several leaves)     */
    const int64_t* values;    /* elided leaf: [instants] its value per instant = the eliding node's max Dac entry
                                 (superchunk.rs:330-334, 426-433); NULL otherwise                                            */
    const int64_t* minmax;    /* [instants][2] stored (min, max) of the node tile that holds this leaf (has_cells,
                                 superchunk.rs:480-493); may be NULL                                                         */
    int32_t encoding;         /* of values / minmax: the node's DCDF_I32 / I64 / F32 / F64                                   */
    uint8_t fractional_bits;  /* of values / minmax: the node's                                                              */
    uint8_t minmax_exact;     /* minmax are exact values of the chunk's stored integers (value search may prune)            */
    uint8_t _pad[2];
} dcdf_raster_tile;
/* `values` and `minmax` are copied to the device here; no pointer is kept.  Lifetime and slab sharing as dcdf_raster_create.
 * DCDF_ERR_BAD_ARG: a wrong tile count, a chunk leaf whose chunk does not cover [row0, row0 + leaf rows) x
 * [col0, col0 + leaf cols) or has the wrong number of instants, an elided leaf without values, a bad encoding, float
 * fractional_bits > 62.  A raster with no chunk leaf at all is valid.  dcdf_raster_fill_window_batch / search_batch /
 * search_values_batch take tiled rasters: elided pieces are written (fill_window) or tested (search) on the device in the same
 * call; the integer search of I32 / I64 rasters drops a piece whose leaf's minmax fails has_cells over the piece's instants
 * (Superchunk::search), the value search prunes with minmax only where minmax_exact is set.  Searches of tiled rasters need
 * k = 2 chunks (DCDF_ERR_UNSUPPORTED otherwise). */
int dcdf_raster_create_tiles(const dcdf_raster_tile* tiles, size_t n_tiles, const uint32_t shape[3], uint32_t tile,
                             uint32_t chunk_size, dcdf_raster** out);
/* Dataset-level points {instant, row, col} (Superchunk::get, superchunk.rs:313-352) / series {start, end, row, col}
 * (Superchunk::fill_cell, superchunk.rs:356-400) in raster coordinates, for every raster, plain or tiled.  One thread per point
 * or series element; the result is typed like dcdf_query_fill_window_batch_typed (out_dtype, out_mem).  get: out[i] = point i.
 * fill_cell: series i (reversed bounds swapped) at out + out_offset[i] (elements; out_offset NULL = the series one after the
 * other).  DCDF_ERR_BOUNDS: a point or series outside the raster. */
int dcdf_raster_get_batch(const dcdf_raster* r, const uint32_t* points, size_t n, void* out, int32_t out_dtype, int out_mem,
                          float* kernel_ms);
int dcdf_raster_fill_cell_batch(const dcdf_raster* r, const uint32_t* cells, size_t n, void* out, int32_t out_dtype,
                                int out_mem, const uint64_t* out_offset, float* kernel_ms);

/* ---- misc ---------------------------------------------------------------------------------- */
/* fixed.rs:96-159 + mmbuffer.rs:596-613: per-tile suggest_fraction on the device; out_round = 1 for
 * Fraction::Round.  Host or device data per `mem`. */
int dcdf_suggest_fraction(const dcdf_tile_desc* tile, int mem, int32_t* out_round, int32_t* out_bits);

/* Bench/test utility: fills dst[(t1-t0)][(r1-r0)][(c1-c0)] (DEVICE memory, dense) with the deterministic
 * synthetic raster of SURVEY.md section 8(d) (same integers as dcdf_amd/synth.py; costab_host = its 1024-entry
 * cosine table).  DCDF_I32 -> v, DCDF_I64 -> 2*v+1. */
int dcdf_synth_fill(void* dst_device, int32_t dtype, uint64_t seed, int64_t t0, int64_t t1, int64_t r0, int64_t r1,
                    int64_t c0, int64_t c1, const int32_t* costab_host);

/* Profiling utility: reads n_tiles dense [instants,256,256] int32 tiles (DEVICE memory) once with the encoder's
 * load pattern, so rocprofv3's FETCH_SIZE can be calibrated against a known byte count (MI355X_MICROARCH.md). */
int dcdf_calib_read(const void* tiles_device, uint32_t n_tiles, uint32_t instants);

/* Device memory for callers that have no HIP binding of their own (the ctypes mirror, tests, tools): hipMalloc /
 * hipFree / hipMemcpy (to_device != 0: host -> device, else device -> host). */
int dcdf_device_alloc(size_t bytes, void** out);
int dcdf_device_free(void* p);
int dcdf_device_copy(void* dst, const void* src, size_t bytes, int to_device);

/* The library keeps a few large device blocks between calls (an appending caller asks for the same sizes slice after
 * slice; hipMalloc / hipFree of gigabytes cost tens of milliseconds).  It gives them back by itself when one of its own
 * allocations fails; a caller that shares the device with another allocator can return them at any time: the bytes freed
 * are stored to *freed_bytes (may be NULL).  Environment K2R_POOL=0 disables the pool. */
int dcdf_device_pool_trim(uint64_t* freed_bytes);

const char* dcdf_strerror(int code);
/* "gfx950 <device name>, <CUs> CUs" or NULL when no device. */
const char* dcdf_device_name(void);
int dcdf_abi_version(void);
/* The raw hipError_t of the last HIP failure seen by this thread (0 = none), for DCDF_ERR_HIP / _HIP_INVALID /
 * _NO_DEVICE / _NOMEM returns. */
int dcdf_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DCDF_K2R_H */
