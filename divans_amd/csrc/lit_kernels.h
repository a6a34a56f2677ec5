// lit_kernels.h -- shared between the HIP kernels and the C-ABI host code (not a public header).
#ifndef DIVANS_LIT_KERNELS_H_
#define DIVANS_LIT_KERNELS_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace divans_hip {

constexpr int LIT_THREADS = 256;    // 4 waves = 16 streams per workgroup
constexpr int RANS_THREADS = 64;    // one wave, one lane per stream

// per-batch constant tables staged in LDS by every workgroup
constexpr uint32_t LIT_BLOB_LUT1CLASS = 0;  // class (<8) of literal_lut1[b]: index of its value among the distinct lut1 values
constexpr uint32_t LIT_BLOB_CTXF = 256;     // [block type][prev][class]: literal_context_map[(lut0[prev] | lut1 value) + 64*btype], literal.rs:97-115
constexpr uint32_t LIT_CTXF_BYTES = 2048;   // one block type's table; n_btypes of them follow each other
constexpr uint32_t LIT_MAX_BTYPES = 8;      // block types one codec keeps FUSED context tables for (LDS: 2 KB each)
// then mixing_mask[8192] at LitGeometry::mix_off = 256 + 2048 * n_btypes
constexpr uint32_t LIT_BLOB_MAX_BYTES = 256 + LIT_CTXF_BYTES * LIT_MAX_BTYPES + 8192;
// The second ("wide") layout, for n_btypes > LIT_MAX_BTYPES (up to LIT_WIDE_MAX_BTYPES): lut0 | lut1 is fused once, the context map stays
// a 64-byte row per block type, and the context of a byte is CMAP[t][SEL[prev][k]] -- two dependent LDS byte reads instead of one.
//   [0, 256)           lut1 class of a byte (LIT_BLOB_LUT1CLASS, as above)
//   [256, 2304)        SEL[prev][k] = (lut0[prev] | class_value[k]) & 63; k >= lut1_classes copies class 0, as the fused table does
//   [2304, 2304 + 64n) CMAP[t][sel] = literal_context_map[64 * (bt_first + t) + sel], t < n = n_btypes
//   then mixing_mask[8192] at LitGeometry::mix_off = 2304 + 64 n         (26 880 bytes at 256 types: below LIT_BLOB_ALLOC_BYTES)
// The blob of a codec with more than LIT_MAX_BTYPES types is laid out this way whatever its context map; the KERNELS read it -- the
// WIDE template argument of the streaming kernels -- only where the map is not constant (lit_wide): under a constant context no
// kernel reads a context table, and such a codec keeps the instances it has at eight types.
constexpr uint32_t LIT_BLOB_SEL = 256;
constexpr uint32_t LIT_BLOB_CMAP = LIT_BLOB_SEL + 2048;
constexpr uint32_t LIT_CMAP_BYTES = 64;
constexpr uint32_t LIT_WIDE_MAX_BTYPES = 256;
// what a codec allocates for its blob: the largest fused blob with the high-row slot tables behind it (capi.cpp derive_high_row_slots)
constexpr uint32_t LIT_BLOB_ALLOC_BYTES = LIT_BLOB_MAX_BYTES + LIT_CTXF_BYTES * LIT_MAX_BTYPES;
static_assert(LIT_BLOB_CMAP + LIT_CMAP_BYTES * LIT_WIDE_MAX_BTYPES + 8192 <= LIT_BLOB_ALLOC_BYTES, "the largest wide blob fits the codec's allocation");
// bytes of the configuration blob in front of the mixing mask (LitGeometry::mix_off) for n block types
constexpr uint32_t lit_ctx_table_bytes(uint32_t n_btypes) {
    return n_btypes > LIT_MAX_BTYPES ? LIT_BLOB_CMAP + LIT_CMAP_BYTES * n_btypes : LIT_BLOB_CTXF + LIT_CTXF_BYTES * n_btypes;
}

// How the (3 x 256 x 256) prior cube of LiteralNibblePriors (codec/priors.rs:35-37) is compacted for
// one configuration: only the planes / context columns the configuration can reach are materialised.
struct LitGeometry {
    uint32_t nctx;        // number of context-map output values (columns of the high-nibble table)
    uint32_t low_width;   // 16, or 256 when some mixing value is 1 (index_c carries context bits)
    uint32_t plane0, plane1, plane2;  // compact plane index of t = (mm>>7)^(opt_1_f_mask>>2)
    uint32_t low_base;    // first row of the low-nibble table
    uint32_t cm_base;     // first row of LiteralCommandPriorsCM (FirstNibble then SecondNibble)
    uint32_t total_rows;  // rows per stream
    int32_t mm_uniform;   // the mixing value when every reachable entry is equal, else -1
    int32_t ctx_const;    // the context when the context map is constant, else -1
    int32_t inc0, lim0, inc1, lim1, inc2, lim2, inc3, lim3;  // literal_adaptation Speeds (scalars: no dynamic indexing of kernargs)
    uint32_t bt_first, n_btypes;   // context tables exist for literal block types [bt_first, bt_first + n_btypes)
    uint32_t mix_off;              // byte offset of mixing_mask inside the configuration blob
    uint32_t lut1_classes;         // distinct literal_lut1 values of the prediction mode (1 for LSB6 / MSB6: the context is a function of prev alone)
    uint32_t hs_classes;           // > 0: the high-nibble stride table holds [row slot of the lut1 class of prev_prev][prev] (that many slots) instead of
                                   // [ctx][prev] -- the rows a stride-1 configuration can reach; the slots are in LIT_BLOB_CTXF[prev][4 + class]
    uint32_t wrap_check;           // some speed lets a row total leave i16 (divans_gpu_speed_supported is false): streaming kernels without
                                   // row caches, which keep such a row recognisable and report a stream that codes with one (lit_kernels.hip blend_row)
};

// The kernels of a launch read the wide layout (no field says so: it follows from the geometry, and is a template argument on the device)
inline bool lit_wide(const LitGeometry& g) { return g.n_btypes > LIT_MAX_BTYPES && g.ctx_const < 0; }

// One Literal command of a general stream (codec/mod.rs:711-792): `len` literal bytes coded with the literal block type
// `btype` (BlockSwitchLiteral, codec/interface.rs:289-292) after last_8_literals has been reloaded from the ring buffer
// (the 8 output bytes before the command, newest in bits 56..63; codec/mod.rs:771-783).  Priors, Weights and the rANS
// coder run on across segments: a stream's literals are ONE LIT_CODER byte stream.
struct LitSegment { uint32_t len, btype, last8_lo, last8_hi; };

struct LitBatch {
    const uint8_t* blob;        // LIT_BLOB_BYTES of configuration tables
    LitGeometry geom;
    int16_t* tables;            // [resident groups][total_rows][16]
    uint32_t n_streams, stream_len, max_stream_len;
    // encode: literal bytes in, (start|freq<<16) out.  decode: coded bytes in, literal bytes out.
    const uint8_t* in; const uint64_t* in_offsets; const uint32_t* in_sizes;
    uint8_t* out; const uint64_t* out_offsets; const uint32_t* out_sizes;
    uint32_t* sf;               // encode only: [n_streams][2*max_stream_len]
    uint32_t cache_rows_high;   // rows of the per-stream LDS cache for high-nibble rows (power of two >= 16, or 0)
    uint32_t cache_rows_low;    // same for low-nibble rows (ignored when cache_unified)
    uint32_t cache_mode;        // 0 none, 1 unified (cache_rows_high rows serve both tables), 2 high-nibble rows only, 3 separate high / low
    uint32_t cache_bytes_per_wg;  // 16 * (rows_high + rows_low) * (32 + 2)
    const uint32_t* seg_begin;  // [n_streams + 1] first segment of every stream in `segs`, or null: each stream is one segment
    const LitSegment* segs;     //   with zero context and the block type the tables were built for
    uint32_t* status;           // device word: bit 0 = encoder saw an invalid (start,freq), bit 1 = decoder integrity check failed
    // lit_decode2.hip: four direct-mapped row caches per stream (high stride rows, high context-map rows, low stride rows, low
    // context-map rows), one byte each: log2(rows) + 1, 0 = that table is not cached; and the hash shift of each
    // (set = (row ^ (row >> shift)) & (rows - 1)).  cache_bytes_per_wg then covers the word rings too.  Bit 31 of dm_shift selects the
    // 2-way organisation of all four, LIT_DM_PINNED the pinned organisation of the high stride rows (lit_decode2_can_pin): the rows of
    // the byte ranks 0 .. P-1 live in LDS, P = what cache_bytes_per_wg leaves a stream behind its ring / 32.
    uint32_t dm_log2, dm_shift;
    uint8_t* stream_bad;        // optional [n_streams]: set to 1 for every stream whose decode failed its integrity check
    // lit_model_encode_kernel, one stream coded piece by piece (divans_gpu_lit_stream_*): `resume` = this launch continues the
    // stream of the previous one -- its CDF tables are kept (no row cache: cache_mode 0), the two Weights objects come back from
    // `wstate` ([2][3] ints: model_weights[1], [0]) -- and every launch leaves them there; the history arrives as a segment's last8
    uint32_t resume; int32_t* wstate;
    // lit_decode_kernel under `resume` / `wstate` likewise (whole chunks per launch: a chunk starts from fresh rANS states, so nothing
    // else carries over); `consumed` (optional, [n_streams]) receives the coded words a stream read, and with it set the words
    // offered may outnumber the words read (the caller passes what has arrived so far)
    uint32_t* consumed;
    // lit_decode2.hip, stride-1 instances: the order in which a table lays out the rows of the 256 previous-byte values -- a device
    // array of 256 ranks (a permutation: the codec learns it from the bytes it has seen, divans_gpu_codec_set_byte_order), or null =
    // numeric.  A private layout of the launch: any order decodes the same bytes.
    const uint8_t* byte_rank;
};
constexpr uint32_t LIT_DM_PINNED = 1u << 30;

// One command of a general stream as the decoder executes it (divans_lit_command of include/divans_gpu.h): LITERAL decodes `len` bytes
// under the block type `arg`, COPY repeats `len` bytes from `arg` bytes back, INSERT takes `len` bytes at offset `arg` of the stream's
// insert bytes (a dictionary word the host has expanded and transformed).  The kinds are the reference's command nibbles.
struct LitCommand { uint32_t kind, len, arg, reserved; };
constexpr uint32_t LIT_CMD_COPY = 0u, LIT_CMD_INSERT = 1u, LIT_CMD_LITERAL = 3u;
// The lists of a batch decoded from its commands (launch_decode2_commands): LitBatch::out / out_offsets / out_sizes are then the
// streams' RAW ranges and `lit_sizes` their literal bytes; LitBatch::seg_begin / segs stay null
struct LitCommandLists {
    const uint32_t* cmd_begin;  // [n_streams + 1] first command of every stream in `cmds`
    const LitCommand* cmds;
    const uint32_t* lit_sizes;  // [n_streams] literal bytes the stream's coded bytes hold
    const uint8_t* ins; const uint64_t* ins_offsets; const uint32_t* ins_sizes;   // insert bytes of every stream, or all null
    // History (divans_gpu_lit_decode_commands_history_batch), or all null: the hist_sizes[s] bytes at hist + hist_offsets[s] lie logically
    // in front of stream s's output -- a COPY may reach into them, a Literal command near the stream's start takes its context from
    // them.  Only read; the ranges of different streams may overlap (a shared dictionary), none may meet a raw range of the launch.
    const uint8_t* hist; const uint64_t* hist_offsets; const uint32_t* hist_sizes;
};
// The step in front of the segment encoders for a batch ENCODED from its commands (lit_commands.hip, launch_commands_prepare): stream
// s = raw + raw_offsets[s], raw_sizes[s] bytes at any alignment, commands cmds[cmd_begin[s] .. cmd_begin[s + 1]), insert bytes as in
// LitCommandLists.  The kernel checks every command, compares what the COPY and INSERT commands would produce with the raw bytes, and
// leaves what divans_gpu_lit_encode_segments_batch takes: the literals of stream s at lit + s * lit_slot (lit_offsets[s], lit_sizes[s]),
// its segments at segs[seg_begin[s] .. seg_begin[s + 1]), one per Literal command with bytes (a count kernel and a one-workgroup scan
// fill seg_begin first).  A stream whose list cannot run or does not reproduce the raw bytes raises LIT_STATUS_BAD_COMMAND /
// LIT_STATUS_BAD_SEGMENT, sets stream_bad[s] and is left as a stream without literals: empty segments only, lit_sizes[s] = 0.
struct LitCommandPrepare {
    const uint8_t* raw; const uint64_t* raw_offsets; const uint32_t* raw_sizes;
    uint32_t n_streams, lit_stream_len;
    const uint32_t* cmd_begin; const LitCommand* cmds;
    uint32_t cmd_first, cmd_last;   // cmd_begin[0], cmd_begin[n_streams] as the host read them: segs holds cmd_last - cmd_first records
    const uint8_t* ins; const uint64_t* ins_offsets; const uint32_t* ins_sizes;   // or all null
    const uint8_t* hist; const uint64_t* hist_offsets; const uint32_t* hist_sizes;   // history as in LitCommandLists, or all null; may lie inside `raw`
    uint32_t bt_first, n_btypes;   // the block types a Literal command may name (LitGeometry)
    uint8_t* lit; uint64_t lit_slot;   // literal slots: lit_stream_len rounded up to 16 bytes each
    uint64_t* lit_offsets; uint32_t* lit_sizes;   // [n_streams]
    uint32_t* seg_begin;            // [n_streams + 1]
    LitSegment* segs;
    uint32_t* out_lit_sizes;        // [n_streams] the caller's copy of lit_sizes
    uint32_t* status; uint8_t* stream_bad;
};
hipError_t launch_commands_prepare(const LitCommandPrepare& b, hipStream_t st);   // count, scan, prepare: three launches

constexpr uint32_t LIT_STATUS_BAD_MODEL = 1u;    // rANS pass: freq == 0 or start/freq outside 15 bits
constexpr uint32_t LIT_STATUS_BAD_SEGMENT = 4u;   // a segment names a literal block type outside the codec's context tables, or a stream's segment lengths do not add up to it
constexpr uint32_t LIT_STATUS_OUTPUT_FULL = 8u;   // divans_gpu_lit_encode_packed: the coded streams did not fit the caller's buffer
constexpr uint32_t LIT_STATUS_BAD_COMMAND = 16u;  // decode from commands: a copy from in front of the stream, an insert outside its bytes, an unknown kind, lengths that do not add up to the raw size
constexpr uint32_t LIT_STATUS_BAD_STREAM = 2u;    // decode: a chunk did not end with both states at 2^31, or the coded words were not consumed exactly

struct RansBatch {
    const uint32_t* sf; uint32_t n_streams, stream_len, max_stream_len; const uint32_t* in_sizes;
    uint32_t sf_stride;         // u32 elements per stream in sf (a multiple of 4): 2 * max_stream_len, or the work-array slot when the
                                // model pass left the pairs in place (BucketBatch::sfs / MixBucketBatch::xs[0])
    uint64_t out_base;          // added to the offsets written to out_offsets: `out` points at the first slot of a sub-batch
    uint8_t* out; uint64_t out_slot; uint64_t* out_offsets; uint32_t* out_sizes; uint32_t* status;
    uint32_t* chunk_bytes; uint32_t max_chunks;   // optional [n_streams][max_chunks] coded size of every 65 536-symbol chunk
    // chunk-parallel variant (streams of at most two chunks): chunk 0 is coded into scratch + (s + 1) * scratch_stride
    // (right-aligned) and then moved in front of chunk 1; null scratch selects the one-lane-per-stream kernel
    uint8_t* scratch; uint64_t scratch_stride; uint32_t* chunk0_sizes;
    uint32_t split_states;      // chunk-parallel variant: two lanes per chunk, one per rANS state (rans_encode2_split_kernel) -- for batches too small to fill the SIMDs
};

typedef unsigned int bk_u32x2 __attribute__((ext_vector_type(2)));
// Bucketed encoder model pass (lit_bucket.hip): mixing value 4, no mixing, context constant or a function of the previous byte -- or
// one stride distance of 2, 3, 4 or 8 under a constant context (launch_bucket_stride_model: the key is the byte that far back).
// With a segment list only the sort kernel changes: a segment's last8 replaces the bytes before its first position in the bucket keys.
struct BucketBatch {
    const uint8_t* in; const uint64_t* in_offsets; const uint32_t* in_sizes;
    uint32_t n_streams, stream_len, max_stream_len;
    uint32_t pieces;            // 8 KiB pieces per stream slot = ceil(max_stream_len / 8192), at most 8
    uint32_t slot;              // elements per stream in sorted / inv / sfs: pieces * 8192 (+ an optional pad)
    uint32_t sf_stride;         // u32 elements per stream in sf
    uint8_t* sorted;            // [n_streams][pieces * 8192] literal bytes, every piece ordered by (previous byte, position)
    uint16_t* inv;              // [n_streams][pieces * 8192] slot of a position inside its sorted piece
    uint32_t* desc;             // [n_streams][256 previous-byte values][8 pieces] first slot | count << 16
    bk_u32x2* sfs;              // [n_streams][pieces * 8192] (high, low) start|freq<<16 pairs in sorted order
    uint32_t* sf;               // [n_streams][2 * max_stream_len] the same pairs in position order (what rans_encode_kernel reads)
    uint32_t* tasks;            // [6 size classes][n_streams * 256] stream * 256 + previous byte
    uint32_t* counters;         // [0..5] tasks per class, [8] next unclaimed task
    int32_t inc, lim;           // literal_adaptation[0]
    // general streams (bucket_sort_kernel<true>), or null: every stream is one segment with zero history
    const uint32_t* seg_begin;  // [n_streams + 1] first segment of every stream in `segs` (the caller's array, offset like in_offsets)
    const LitSegment* segs;
    uint32_t bt_first, n_btypes;   // the block types a segment may name (LitGeometry); they do not enter the keys
    uint32_t* status;           // device word: LIT_STATUS_BAD_SEGMENT
};
hipError_t launch_bucket_model(const BucketBatch& b, uint32_t chain_blocks, hipStream_t st);
// The same pass keyed by the byte `dist` places back (2, 3, 4 or 8: mixing values 5, 6, 7, and 8 and above, under a constant context):
// bucket_sort_stride_kernel in place of bucket_sort_kernel, every other kernel and every field of the batch as above
hipError_t launch_bucket_stride_model(const BucketBatch& b, uint32_t dist, uint32_t chain_blocks, hipStream_t st);
void launch_bucket_tasks(const BucketBatch& b, hipStream_t st);
void launch_bucket_unsort(const BucketBatch& b, hipStream_t st);
void launch_bucket_unsort32(const BucketBatch& b, hipStream_t st);   // the same for a plane of 4-byte elements

// Bucketed encoder model pass for the two-model configuration (lit_bucket_mix.hip): context map on, every mixing value 4
// (stride 1), dynamic mixing (context_mixing >= 2), one literal block type, streams <= 64 KiB.  With a segment list only the sort
// kernels change: a segment's last8 replaces the two bytes before its first position in the keys and high-row slots.
struct MixBucketBatch {
    const uint8_t* in; const uint64_t* in_offsets; const uint32_t* in_sizes;
    uint32_t n_streams, stream_len, max_stream_len;
    uint32_t pieces;            // 8 KiB pieces per stream slot, at most 8
    uint32_t slot;              // elements per stream in sorted / inv / the record planes (see BucketBatch::slot)
    uint32_t pos_stride;        // elements per stream in xs[] / maxes[]
    uint32_t sf_stride;         // u32 elements per stream in sf
    const uint8_t* blob;        // configuration tables (LIT_BLOB_LUT1CLASS, LIT_BLOB_CTXF of the one block type)
    uint16_t* sorted;           // [n_streams][pieces * 8192] byte | high-row slot << 8, every piece ordered by (key, position)
    uint16_t* inv;              // [n_streams][pieces * 8192] slot of a position inside its sorted piece
    uint32_t* desc;             // [n_streams][256 keys][8 pieces] first slot | count << 16
    uint32_t* tasks;            // [6 size classes][n_streams * 256]
    uint32_t* counters;
    // What the chains leave per position and model (0 stride, 1 context map), taken from the two rows BEFORE they are blended with the
    // position's nibbles: xs[m][n_streams][slot] = {high: cdf[sym] | cdf[sym-1] << 16, low: the same}, maxes[m][n_streams][slot] =
    // cdf[15] of the high row | of the low row << 16 -- 12 bytes, split so that each plane keeps power-of-two elements.  The chains
    // write them in sorted order; the unsort kernels put every piece back into position order in place (a whole piece sits in LDS
    // before it is written).
    bk_u32x2* xs[2];
    uint32_t* maxes[2];
    uint32_t* sf;               // [n_streams][sf_stride] what rans_encode_kernel reads; may be xs[0] (mix_weights_kernel reads a
                                // chunk of all four planes before it writes that chunk's pairs)
    int32_t inc0, lim0, inc2, lim2, inc3, lim3;   // literal_adaptation[0] (stride rows), [2] (cm low), [3] (cm high)
    // general streams (mix_sort_kernel<MODEL, true>), or null; as in BucketBatch
    const uint32_t* seg_begin;
    const LitSegment* segs;
    uint32_t bt_first, n_btypes;
    uint32_t* status;
};
hipError_t launch_bucket_mix_model(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st);

// Bucketed encoder model passes for context-keyed rows (lit_bucket_ctx.hip): a context map that is not constant, every reachable
// mixing value 0, up to LIT_MAX_BTYPES block types, streams <= 64 KiB.  Every row of a position is a function of its context, so one
// sort by ctx = LIT_BLOB_CTXF[block type of the covering segment][prev][class of prev_prev] (ctx_sort_kernel) serves one model or two.
// Both take a MixBucketBatch (blob, segment list, speeds):
//   one model   `sorted` holds bytes (n_streams * slot of them), xs[0] receives the (start | freq << 16) pairs; the other planes are unused
//   two models  as launch_bucket_mix_model, with 16-bit payloads that hold the byte alone
hipError_t launch_bucket_ctx_model(const MixBucketBatch& b, uint32_t chain_blocks, hipStream_t st);
hipError_t launch_bucket_ctx_mix_model(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st);
// what they borrow from the other two passes' files
void launch_bucket_chain(const BucketBatch& b, uint32_t chain_blocks, hipStream_t st);                    // bucket_chain_kernel
void launch_mix_chain_ctx(const MixBucketBatch& b, int model, uint32_t num_cus, hipStream_t st);         // model 0: mix_chain_ctx_kernel<0>, 1: mix_chain_kernel<1>
void launch_mix_weights(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st);                      // mix_weights_kernel<1 | 2>

// Bucketed two-model pass for SEVERAL literal block types (lit_bucket_ctx.hip): context map on, every mixing value 4, dynamic mixing,
// up to LIT_MAX_BTYPES block types of which no previous byte reaches more than eight contexts, streams <= 64 KiB.  The stride model's
// buckets stay keyed by prev and the block type of the covering segment enters the payload's high-row slot (mix_bt_sort_kernel reads
// the slot tables the host put behind the mixing mask: blob + LIT_BLOB_CTXF + LIT_CTXF_BYTES * n_btypes + 8192); the context model's
// sort is ctx_sort_kernel<true, SEG>.  Chains, task lists, unsorts and the Weights walk are launch_bucket_mix_model's.
hipError_t launch_bucket_mix_bt_model(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st);
void launch_mix_chain(const MixBucketBatch& b, int model, uint32_t num_cus, hipStream_t st);             // mix_chain_kernel<0 | 1> (lit_bucket_mix.hip)

uint32_t lit_lds_bytes(const LitBatch& b);
hipError_t launch_model_encode(const LitBatch& b, bool mix, uint32_t blocks, hipStream_t st);
hipError_t launch_rans_encode(const RansBatch& b, hipStream_t st);
hipError_t launch_decode(const LitBatch& b, bool mix, uint32_t blocks, hipStream_t st);
hipError_t launch_decode2(const LitBatch& b, bool mix, uint32_t blocks, hipStream_t st);
// lit_decode2_kernel with the stream's Copy / Insert commands executed on the device (lit_decode2_cmd_kernel_*): b.dm_log2 = what
// lit_decode2_commands_caches() leaves, the 2-way organisation whatever b.dm_shift says
hipError_t launch_decode2_commands(const LitBatch& b, const LitCommandLists& cl, bool mix, uint32_t blocks, hipStream_t st);
void lit_decode2_commands_kernel_name(const LitBatch& b, bool mix, bool hist, char* buf, size_t cap);   // hist: the lists come with a history (lit_decode2_cmd_hist_kernel)
uint32_t lit_decode2_commands_caches(uint32_t dm_log2, bool mix, uint32_t total_rows);   // the high-row caches of dm_log2, or none
void lit_decode_kernel_name(const LitBatch& b, bool mix, char* buf, size_t cap);    // the instances the two launchers pick, as rocprofv3 spells them
void lit_decode2_kernel_name(const LitBatch& b, bool mix, char* buf, size_t cap);
uint32_t lit_decode2_effective_caches(uint32_t dm_log2, bool mix, bool seg);   // the caches of dm_log2 a kernel instance exists for
uint32_t lit_decode2_stream_lds(uint32_t dm_log2, bool pinned = false);   // LDS bytes one stream takes in lit_decode2_kernel (word ring + row caches: 34 bytes per tagged row, 32 per pinned one)
bool lit_decode2_can_pin(const LitBatch& b, bool mix);    // a pinned instance exists for this launch (b.geom, b.segs and b.dm_log2 are read)
// Decoders that lost their measurement and are NOT part of the default library (build with DIVANS_WITH_EXPERIMENTAL_DECODERS=1 in the
// environment of divans_amd/build.py to have them): generation 4 = lit_decode_t.hip, one lane per stream, 30-45 % slower everywhere
// (profiles/r04e_lane_per_stream_decoder.txt), and the instances of generation 1's lit_decode_kernel no product path needs (the unified and
// split cache organisations; 3-8 % behind generation 3, profiles/r03b_bench_decoder_generations_same_box.txt).  Generation 1 without a
// cache / with the high-row cache stays: it decodes under speeds whose row totals leave i16 (wrap-checked) and call by call (resumable).
#ifndef DIVANS_WITH_EXPERIMENTAL_DECODERS
#define DIVANS_WITH_EXPERIMENTAL_DECODERS 0
#endif
#if DIVANS_WITH_EXPERIMENTAL_DECODERS
// lit_decode_t.hip: one lane per stream (decoder generation 4); 64 streams per workgroup
hipError_t launch_decode_t(const LitBatch& b, bool mix, uint32_t blocks, hipStream_t st);
hipError_t launch_selftest_cdf_ops_t(const uint32_t* d_ops, uint32_t n, int32_t* d_out, hipStream_t st);   // the selftest script on its arithmetic
void lit_decode_t_kernel_name(const LitBatch& b, bool mix, char* buf, size_t cap);
uint32_t lit_decode_t_stream_lds(uint32_t dm_log2, bool mix);   // LDS bytes one stream takes there
#endif
hipError_t launch_pack(const uint8_t* slots, const uint64_t* src_off, const uint32_t* sizes, uint32_t n, uint8_t* packed,
                       uint64_t* dst_off, uint64_t* total, hipStream_t st, bool accumulate = false, uint64_t cap = ~0ull, uint32_t* status = nullptr);
// rank[b] = position of byte value b when the 256 values are ordered by how often they occur in a sample of the batch (the first
// `sample_len` bytes of `sample_streams` streams spread over it), ties by value: one workgroup, enqueued behind the launch that
// produced / consumed the bytes (lit_decode2.hip)
hipError_t launch_learn_byte_rank(const uint8_t* data, const uint64_t* offsets, const uint32_t* sizes, uint32_t n_streams, uint32_t stream_len,
                                  uint32_t sample_streams, uint32_t sample_len, uint8_t* rank, hipStream_t st);
// The decoder's row traffic without the decoder: the streams' bytes are KNOWN (b.in = the literal bytes, in_offsets / in_sizes theirs),
// every row the decoder of this configuration would touch is loaded, blended with the byte's nibble and stored through the same
// per-stream LDS caches, table layout and persistent grid -- no rANS state, no search, no division, nothing that makes one byte wait
// for the previous one except the rows themselves.  Its time is the memory side's own ceiling for this access stream (bench.py:
// roofline.request_ceiling).  Leaves the tables as a decode of the same bytes would; writes nothing else.
hipError_t launch_row_replay(const LitBatch& b, bool mix, uint32_t blocks, hipStream_t st);
hipError_t launch_selftest_division(unsigned long long* d_mismatches, hipStream_t st);
hipError_t launch_selftest_cdf_ops(const uint32_t* d_ops, uint32_t n, int32_t* d_out, hipStream_t st);
// the same script on the arithmetic of lit_decode2.hip / of the bucketed encoder passes (lit_bucket_dev.h, lit_bucket_mix.hip)
hipError_t launch_selftest_cdf_ops2(const uint32_t* d_ops, uint32_t n, int32_t* d_out, hipStream_t st);
hipError_t launch_selftest_cdf_ops_bucket(const uint32_t* d_ops, uint32_t n, int32_t* d_out, hipStream_t st);

}  // namespace divans_hip
#endif
