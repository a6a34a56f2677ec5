// lit_bucket_mix.hip -- bucketed model pass of the ENCODER for the two-model configuration (BASELINE configs[2],
// reference TestContextMixing, bin/benchmark.rs:156-167): context map on, every mixing value 4, dynamic mixing.
//
// Each nibble is coded with the weighted average of two rows (codec/literal.rs:209-241):
//   stride model   high nibble: row [ctx][prev]      low nibble: row [prev][hi]       blended with literal_adaptation[0]
//   context model  high nibble: row First[ctx]       low nibble: row Second[hi][ctx]  blended with literal_adaptation[3] / [2]
// and the weights of the average follow from how well each model did on the symbols before (codec/weights.rs:23-38).
// A row's CDF depends only on the earlier positions that used the same row -- never on the weights -- so the rows
// can be walked bucket by bucket exactly as in lit_bucket.hip, once per model (the chain loop of both models is bk_chain_loop, lit_bucket_dev.h):
//   stride model:  buckets keyed by prev  (up to 8 high rows, one per class of prev_prev that reaches a different ctx, + 16 low rows)
//   context model: buckets keyed by ctx   (1 high row + 16 low rows)
// Instead of (start, freq) a chain lane leaves the three raw counts mixing needs per nibble -- cdf[sym], cdf[sym-1], cdf[15] --
// as 12 bytes per position: {high: cdf[sym] | cdf[sym-1] << 16, low: the same} in one plane, the two cdf[15] in another.
// After both models' records are back in position order, mix_weights_kernel runs the only serial part that is left --
// the per-stream Weights recursion, one lane per (stream, nibble half): average (probability/frequentist_cdf.rs:58-72)
// of the three entries, the six divisions of sym_to_start_and_freq (probability/interface.rs:97-108), Weights::update.
#include "lit_bucket_dev.h"

namespace divans_hip {

// Chain waves per CU.  The stride model's 24 rows per lane allow three; the context model's 17 would allow four, but three
// were faster in round 2 (30.9 vs 35.7 ms per 32 768 streams, two: 32.2): with 16 bytes of records leaving per lane and step the
// waves of a CU queue up behind its vector-memory path (TA busy 80 %), and a fourth wave only lengthens the queue.  With the
// 16-byte payload loads of round 3 three and four measure the same.
constexpr uint32_t MX_CHAIN_WAVES = 3;

template <int MODEL> struct MxGeom {
    static constexpr uint32_t NH = MODEL == 0 ? 8u : 1u;            // high-nibble rows of a bucket
    static constexpr uint32_t NR = NH + 16u;
    // rows + 8 descriptors, padded so that the 64 lanes' b128 accesses at equal offsets cover all 32 banks
    static constexpr uint32_t LANE_DW = MODEL == 0 ? 204u : 148u;
    static constexpr uint32_t LDS_BYTES = (64u * LANE_DW + 256u) * 4u;
};

// ---------------------------------------------------------------------------------------------
// 1. per (stream, piece): sorted[slot] = byte | high-row slot << 8, inv[pos] = slot, desc[stream][key][piece]
//    MODEL 0 (stride): key = prev.  MODEL 1 (context map): key = ctx (literal.rs:87-117 through the fused table).
//    SEG: the stream has a segment list: the first byte of every non-empty segment takes prev and prev_prev from the segment's last8,
//    its second byte prev_prev (SegCursor, lit_device.h).  The keys are first formed from the bytes themselves, then the workgroup
//    walks the list (bk_seg_walk) and forms those two positions' keys again, and only then counts them; the workgroup of piece 0
//    checks the list.  SEG = false is the code it was.
// ---------------------------------------------------------------------------------------------
template <int MODEL, bool SEG>
__global__ __launch_bounds__(BK_SORT_THREADS) void mix_sort_kernel(const MixBucketBatch b) {
    __shared__ __attribute__((aligned(16))) uint16_t staging[BK_PIECE];
    __shared__ __attribute__((aligned(16))) uint8_t piece_in[16 + BK_PIECE];   // piece_in[14], [15] = the two bytes before the piece
    __shared__ uint16_t kp[BK_PIECE];                                          // key | high-row slot << 8 of every position
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t scan[256];
    __shared__ uint8_t lut1c[256], ctxf[2048], slot_of[2048];
    const uint32_t s = blockIdx.x / b.pieces, piece = blockIdx.x % b.pieces;
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint32_t len = b.in_sizes ? b.in_sizes[s] : b.stream_len;
    const uint8_t* in = b.in + (b.in_offsets ? b.in_offsets[s] : (uint64_t)s * b.stream_len);
    uint32_t* desc = b.desc + ((size_t)s * 256u + tid) * 8u + piece;
    const uint32_t base = piece * BK_PIECE;
    if (base >= len) {
        *desc = 0u;
        if (SEG && piece == 0u)     // an empty stream: its list still has to add up to it
            bk_seg_walk(b.seg_begin, b.segs, s, 0u, ~0u, true, b.bt_first, b.n_btypes, b.status, scan, [](uint32_t, uint32_t, uint64_t) {});
        return;
    }
    const uint32_t n = len - base < BK_PIECE ? len - base : BK_PIECE;
    const size_t pl = b.slot;
    for (uint32_t i = tid; i < 1024u; i += BK_SORT_THREADS) (&hist[0][0])[i] = 0u;
    lut1c[tid] = b.blob[LIT_BLOB_LUT1CLASS + tid];
    for (uint32_t i = tid; i < 2048u; i += BK_SORT_THREADS) ctxf[i] = b.blob[LIT_BLOB_CTXF + i];
    bk_load_piece(piece_in, in + base, n);
    if (tid == 0u) { piece_in[15] = base ? in[base - 1u] : 0u; piece_in[14] = base ? in[base - 2u] : 0u; }   // last_8_literals starts at zero
    __syncthreads();
    // classes of prev_prev that reach the same context share a high row: slot = the first such class
    if (MODEL == 0) {
        for (uint32_t i = tid; i < 2048u; i += BK_SORT_THREADS) {
            const uint32_t row = i & ~7u; const uint8_t c = ctxf[i];
            uint32_t k = 0; while (ctxf[row + k] != c) ++k;
            slot_of[i] = (uint8_t)k;
        }
        __syncthreads();
    }
    // wave w owns positions [2048 w, 2048 w + 2048) of the piece and visits them in order, 64 at a time
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        const uint32_t p = w * 2048u + bt * 64u + lane;
        if (p < n) {
            const uint32_t prev = piece_in[15u + p], e = (prev << 3) + lut1c[piece_in[14u + p]];
            const uint32_t key = MODEL == 0 ? prev : ctxf[e];
            kp[p] = (uint16_t)(key | (MODEL == 0 ? (uint32_t)slot_of[e] << 8 : 0u));
            if (!SEG) atomicAdd(&hist[w][key], 1u);
        }
    }
    __syncthreads();
    if (SEG) {
        const auto kp_of = [&](uint32_t prev, uint32_t prev_prev) -> uint16_t {
            const uint32_t e = (prev << 3) + lut1c[prev_prev];
            return (uint16_t)((MODEL == 0 ? prev : (uint32_t)ctxf[e]) | (MODEL == 0 ? (uint32_t)slot_of[e] << 8 : 0u));
        };
        // a segment of one byte leaves its second position to the segment that follows: every position is written by one lane at most
        bk_seg_walk(b.seg_begin, b.segs, s, len, piece == 0u ? ~0u : base + n, piece == 0u, b.bt_first, b.n_btypes, b.status, scan,
                    [&](uint32_t q, uint32_t l, uint64_t l8) {
                        const uint32_t newest = (uint32_t)(l8 >> 56), before = (uint32_t)(l8 >> 48) & 0xffu;
                        const uint32_t p = q - base, p1 = q + 1u - base;
                        if (p < n) kp[p] = kp_of(newest, before);
                        if (l >= 2u && p1 < n) kp[p1] = kp_of(piece_in[15u + p1], newest);
                    });
        __syncthreads();
        for (uint32_t bt = 0; bt < 32u; ++bt) {
            const uint32_t p = w * 2048u + bt * 64u + lane;
            if (p < n) atomicAdd(&hist[w][kp[p] & 0xffu], 1u);
        }
        __syncthreads();
    }
    const uint32_t c0 = hist[0][tid], c1 = hist[1][tid], c2 = hist[2][tid], c3 = hist[3][tid];
    const uint32_t tot = c0 + c1 + c2 + c3;
    scan[tid] = tot;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const uint32_t v = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const uint32_t start = scan[tid] - tot;
    hist[0][tid] = start; hist[1][tid] = start + c0; hist[2][tid] = start + c0 + c1; hist[3][tid] = start + c0 + c1 + c2;
    *desc = start | (tot << 16);
    __syncthreads();
    uint16_t* inv = b.inv + (size_t)s * pl + base;
    for (uint32_t bt = 0; bt < 32u; ++bt) {
        const uint32_t p = w * 2048u + bt * 64u + lane;
        const bool valid = p < n;
        const uint32_t k = valid ? kp[p] : 0u;
        const uint32_t key = k & 0xffu;
        const uint32_t pay = valid ? (uint32_t)piece_in[16u + p] | (k & 0xff00u) : 0u;
        unsigned long long same = __ballot(valid);
        for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool set = (key >> bit) & 1u;
            const unsigned long long bb = __ballot(set);
            same &= set ? bb : ~bb;
        }
        const uint32_t rank = lanes_below(same), cnt = (uint32_t)__popcll(same);
        if (valid) {
            const uint32_t off = hist[w][key];
            staging[off + rank] = (uint16_t)pay;
            inv[p] = (uint16_t)(off + rank);
            if (rank == cnt - 1u) hist[w][key] = off + cnt;   // the wave's LDS accesses stay in program order
        }
    }
    __syncthreads();
    uint16_t* sorted = b.sorted + (size_t)s * pl + base;
    for (uint32_t i = tid * 8u; i < n; i += BK_SORT_THREADS * 8u) {
        if (i + 8u <= n) *(u32x4*)(sorted + i) = *(const u32x4*)(staging + i);
        else for (uint32_t k = i; k < n; ++k) sorted[k] = staging[k];
    }
}

// ---------------------------------------------------------------------------------------------
// 3. chains: one lane per bucket, rows in LDS, raw counts out.  The loop is bk_chain_loop (lit_bucket_dev.h, where the reasons for
//    its shape are), one text for both models; this is mix_chain_kernel's part of it: a group is eight 16-bit payloads (one
//    16-byte load), a position leaves its {high, low} entries and its two row totals, two planes are stored.
// ---------------------------------------------------------------------------------------------
template <int MODEL> struct MxChain {
    using G = MxGeom<MODEL>;
    typedef u32x4 Group;
    static constexpr uint32_t ROWS = G::NR;
    struct Env { uint32_t* my; const uint32_t* tabh; const uint32_t* tabl; int limh, liml; };
    struct Slot { u32x2* x; uint32_t* m; };
    struct Out {
        u32x2 x0, x1, x2, x3, x4, x5, x6, x7;                  // {high, low} entries of the group's positions
        uint32_t t0, t1, t2, t3, t4, t5, t6, t7;               // their row totals, high | low << 16
    };
    static __device__ __forceinline__ Slot slot(const MixBucketBatch& b, size_t off) { return {b.xs[MODEL] + off, b.maxes[MODEL] + off}; }
    static __device__ __forceinline__ void store(Slot to, uint32_t m, Out o) {
        bk_store_group(to.x, m, o.x0, o.x1, o.x2, o.x3, o.x4, o.x5, o.x6, o.x7);
        bk_store_group(to.m, m, o.t0, o.t1, o.t2, o.t3, o.t4, o.t5, o.t6, o.t7);
    }
#define MX_POS(K, WORD, RX, RT)                                                                         \
    if (((K - first) & 15u) < cnt) {                                                                    \
        const uint32_t pay = (WORD >> (16u * (K & 1u))) & 0xffffu;                                      \
        const uint32_t hi = (pay >> 4) & 15u, lo = pay & 15u;                                           \
        uint32_t* rowh = MODEL == 0 ? my + ((pay >> 5) & 0x38u) : my;   /* 8 dwords x slot (bits 8..10) */ \
        uint32_t* rowl = my + 8u * (G::NH + hi);                                                        \
        BkRow H = bk_read(rowh, tabh, hi), L = bk_read(rowl, tabl, lo);                                 \
        const u32x2 vx = {(uint32_t)H.chi | (hi ? (uint32_t)H.cprev << 16 : 0u),                        \
                          (uint32_t)L.chi | (lo ? (uint32_t)L.cprev << 16 : 0u)};                       \
        const uint32_t vt = (H.w1.w >> 16) | (L.w1.w & 0xffff0000u);                                    \
        bk_add(H); bk_add(L);                                                                           \
        bk_renorm_at(H, limh); bk_renorm_at(L, liml);                                                   \
        *(u32x4*)rowh = H.w0; *(u32x4*)(rowh + 4) = H.w1; *(u32x4*)rowl = L.w0; *(u32x4*)(rowl + 4) = L.w1; \
        RX = vx; RT = vt;                                                                               \
    }
    static __device__ __forceinline__ Out code(const Env v, const u32x4 e, const uint32_t first, const uint32_t cnt, Out o) {
        uint32_t* const my = v.my; const uint32_t* const tabh = v.tabh; const uint32_t* const tabl = v.tabl; const int limh = v.limh, liml = v.liml;
        MX_POS(0u, e.x, o.x0, o.t0) MX_POS(1u, e.x, o.x1, o.t1) MX_POS(2u, e.y, o.x2, o.t2) MX_POS(3u, e.y, o.x3, o.t3)
        MX_POS(4u, e.z, o.x4, o.t4) MX_POS(5u, e.z, o.x5, o.t5) MX_POS(6u, e.w, o.x6, o.t6) MX_POS(7u, e.w, o.x7, o.t7)
        return o;
    }
#undef MX_POS
};

template <int MODEL>
__global__ __launch_bounds__(64) void mix_chain_kernel(const MixBucketBatch b) {
    using G = MxGeom<MODEL>;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
    const uint32_t lane = threadIdx.x;
    uint32_t* my = lds32 + lane * G::LANE_DW;
    uint32_t* tabh = lds32 + 64u * G::LANE_DW;
    uint32_t* tabl = tabh + 128u;
    const uint32_t inch = (uint32_t)(MODEL == 0 ? b.inc0 : b.inc3), incl = (uint32_t)(MODEL == 0 ? b.inc0 : b.inc2);   // literal.rs:320,354 / :242
    const int limh = MODEL == 0 ? b.lim0 : b.lim3, liml = MODEL == 0 ? b.lim0 : b.lim2;
    for (uint32_t i = lane; i < 128u; i += 64u) {
        tabh[i] = bk_tab_entry(i, inch);
        tabl[i] = bk_tab_entry(i, incl);
    }
    __syncthreads();
    const typename MxChain<MODEL>::Env env = {my, tabh, tabl, limh, liml};
    bk_chain_loop<MxChain<MODEL>>(env, b);
}

// ---------------------------------------------------------------------------------------------
// 5. the Weights recursion: one lane per (stream, nibble half).  model_weights[1] belongs to the high nibbles and
//    model_weights[0] to the low nibbles (literal.rs:230), so the two halves of a stream are independent.
// ---------------------------------------------------------------------------------------------
// entry 15 of the mixed row: both rows contribute their own total, so the two products are equal, rs = ro = (cmax * smax) >> sh, and
// (rs * mix + rs * (2^15 - mix) + 1) >> 15 = rs whatever the weight -- the third average costs a multiply and a shift
__device__ __forceinline__ int mix_total(int cmax, int smax) {
    const uint32_t prod = __umul24((uint32_t)cmax, (uint32_t)smax);
    int lz = __clz((int)prod);
    lz = lz > 17 ? 17 : lz;
    return (int)(prod >> (17 - lz));
}

// REC (the selftest interpreter): also hands back the two model frequencies the Weights update took, cm | stride << 16
template <bool REC = false>
__device__ __forceinline__ uint32_t mix_nibble(Weights& w, uint32_t st_x, uint32_t st_max, uint32_t cm_x, uint32_t cm_max, uint32_t* model_freqs = nullptr) {
    const int mix_rate = w.norm;
    const int cm_s = (int)(cm_x & 0xffffu), cm_p = (int)(cm_x >> 16), st_s = (int)(st_x & 0xffffu), st_p = (int)(st_x >> 16);
    const int cmax = (int)cm_max, smax = (int)st_max;
    const int p_s = average_rows(cm_s, st_s, cmax, smax, mix_rate);       // frequentist_cdf.rs:58-72, entry sym
    const int p_p = average_rows(cm_p, st_p, cmax, smax, mix_rate);       //   entry sym-1 (0 | 0 -> 0 when sym == 0)
    const int pmax = mix_total(cmax, smax);
    const float rp = biased_rcp15(pmax), rc = biased_rcp15(cmax), rs = biased_rcp15(smax);
    const uint32_t qp = scaled_div(p_p, pmax, rp);
    const uint32_t freq = scaled_div(p_s, pmax, rp) - qp - 1u;            // probability/interface.rs:97-108
    const uint32_t fcm = scaled_div(cm_s, cmax, rc) - scaled_div(cm_p, cmax, rc) - 1u;
    const uint32_t fst = scaled_div(st_s, smax, rs) - scaled_div(st_p, smax, rs) - 1u;
    if (REC) *model_freqs = (fcm & 0xffffu) | (fst << 16);
    weights_update(w, (int)(short)fcm, (int)(short)fst, (int)(short)freq);   // literal.rs:236-239
    return (qp + 1u) | (freq << 16);
}

// One wave = 32 streams x 2 halves.  The records of a stream are contiguous in memory, so the wave fetches them
// together -- every 16-byte load instruction covers 128-byte (xs) / 64-byte (maxes) runs of 8 / 16 streams -- into LDS, 16 positions
// at a time, double-buffered; each lane then reads its own stream's records from LDS, and the (start, freq) pairs go back out the
// same way (a lane-per-stream walk straight over global memory costs one 16-byte request per lane and load).
constexpr uint32_t MW_CHUNK = 16;                       // positions per LDS buffer (8 and 4 measured 13 % / 25 % worse on the model pass -- before the
                                                        // one-wave-per-SIMD attribute below, so possibly for its reason; not re-measured)
constexpr uint32_t MW_XP = MW_CHUNK / 2u, MW_TP = MW_CHUNK / 4u;     // 16-byte pieces of a stream's chunk: two xs records, four maxes
constexpr uint32_t MW_XS = 64u / MW_XP, MW_TS = 64u / MW_TP;         // streams one load instruction of the wave covers
constexpr uint32_t MW_XG = 32u / MW_XS, MW_TG = 32u / MW_TS;         // such loads per plane
constexpr uint32_t MW_PER_MODEL = MW_XG + MW_TG;
constexpr uint32_t MW_NLOAD = 2u * MW_PER_MODEL;
constexpr uint32_t MW_MODEL_BYTES = MW_CHUNK * 12u;                  // a stream's chunk of one model in LDS: xs (8 B / position), then maxes (4 B)
constexpr uint32_t MW_IN_STRIDE = 2u * MW_MODEL_BYTES + 16u;         // bytes per stream, padded against bank conflicts
constexpr uint32_t MW_OUT_STRIDE = 2u * MW_CHUNK * 4u + 16u;
constexpr uint32_t MW_IN_BYTES = 32u * MW_IN_STRIDE;

// One wave per SIMD, enforced (amdgpu_waves_per_eu): a wave walks its 32 streams' recursions at the SIMD's issue rate and a second
// wave on the same SIMD only halves both, while a 32 768-stream sequence is exactly one wave for each of the chip's 1024 SIMDs.  Left
// to the dispatcher, a CU's four workgroups do not always land on four different SIMDs: round 2's version happened to be safe because
// its 257 registers allowed one wave per SIMD anyway; with 169 the kernel took 39.6 instead of 24.5 ms until this attribute came.
// A sequence of more than 32 768 streams (round 6: 65 536 where the device has room for its work arrays) is two waves for every SIMD --
// the WPE = 2 instance, pinned to exactly that: the second wave issues into the first one's dependency stalls.
template <int WPE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void mix_weights_kernel(const MixBucketBatch b) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_in[2u * MW_IN_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t lds_out[32u * MW_OUT_STRIDE];
    const uint32_t lane = threadIdx.x;
    const uint32_t s0 = blockIdx.x * 32u;
    // consumer role: stream s0 + lane / 2, nibble half lane & 1
    const uint32_t half = lane & 1u;
    // mover role, xs: stream s0 + 8 g + lane / 8 of load g, records 2 (lane & 7), + 1 of the chunk; maxes: stream s0 + 16 g + lane / 4,
    // totals 4 (lane & 3) .. + 3; pairs out: as xs
    const uint32_t xq = lane % MW_XP, xj = lane / MW_XP, tq = lane % MW_TP, tj = lane / MW_TP;
    const uint32_t chunks = (b.stream_len + MW_CHUNK - 1u) / MW_CHUNK;     // stream_len = the longest stream of the batch
    Weights w; w.w0 = 1; w.w1 = 1; w.norm = 1 << 14;               // weights.rs:15-21
    u32x4 r[MW_NLOAD];
#define MW_FETCH(C)                                                                                     \
    _Pragma("unroll") for (uint32_t i = 0; i < MW_NLOAD; ++i) {                                         \
        const uint32_t model = i / MW_PER_MODEL, g = i % MW_PER_MODEL;                                  \
        if (g < MW_XG) {                                                                                \
            const uint32_t j = g * MW_XS + xj, p = (C) * MW_CHUNK + 2u * xq;                            \
            const bool ok = s0 + j < b.n_streams && p < b.max_stream_len;                               \
            const u32x2* src = b.xs[model] + (ok ? (size_t)(s0 + j) * b.pos_stride + p : 0u);           \
            r[i] = __builtin_nontemporal_load((const u32x4*)src);                                       \
        } else {                                                                                        \
            const uint32_t j = (g - MW_XG) * MW_TS + tj, p = (C) * MW_CHUNK + 4u * tq;                  \
            const bool ok = s0 + j < b.n_streams && p < b.max_stream_len;                               \
            const uint32_t* src = b.maxes[model] + (ok ? (size_t)(s0 + j) * b.pos_stride + p : 0u);     \
            r[i] = __builtin_nontemporal_load((const u32x4*)src);                                       \
        }                                                                                               \
    }
#define MW_STAGE(BUF)                                                                                   \
    _Pragma("unroll") for (uint32_t i = 0; i < MW_NLOAD; ++i) {                                         \
        const uint32_t model = i / MW_PER_MODEL, g = i % MW_PER_MODEL;                                  \
        uint8_t* dst = lds_in + (BUF) * MW_IN_BYTES + model * MW_MODEL_BYTES;                           \
        if (g < MW_XG) *(u32x4*)(dst + (g * MW_XS + xj) * MW_IN_STRIDE + xq * 16u) = r[i];              \
        else *(u32x4*)(dst + ((g - MW_XG) * MW_TS + tj) * MW_IN_STRIDE + MW_CHUNK * 8u + tq * 16u) = r[i]; \
    }
    if (chunks == 0u) return;
    MW_FETCH(0u)
    MW_STAGE(0u)
    __syncthreads();
    const uint32_t hs = 16u * half;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t buf = c & 1u;
        if (c + 1u < chunks) { MW_FETCH(c + 1u) }
        const uint8_t* mine = lds_in + buf * MW_IN_BYTES + (lane >> 1) * MW_IN_STRIDE;
        uint32_t* outp = (uint32_t*)(lds_out + (lane >> 1) * MW_OUT_STRIDE) + half;
        const uint32_t p0 = c * MW_CHUNK;
#pragma unroll
        for (uint32_t k = 0; k < MW_CHUNK / 2u; ++k) {
            const u32x4 st = *(const u32x4*)(mine + k * 16u), cm = *(const u32x4*)(mine + MW_MODEL_BYTES + k * 16u);
            const u32x2 stt = *(const u32x2*)(mine + MW_CHUNK * 8u + k * 8u), cmt = *(const u32x2*)(mine + MW_MODEL_BYTES + MW_CHUNK * 8u + k * 8u);
            // No test against the stream's length: past its end the walk chews on whatever the staging buffers hold (loads are clamped to
            // mapped memory, integer arithmetic does not trap), its Weights are never used again and the pairs are not stored (the
            // store-out below tests the length) -- and without 32 branches per chunk the compiler schedules across positions.
            outp[4u * k] = mix_nibble(w, half ? st.y : st.x, (stt.x >> hs) & 0xffffu, half ? cm.y : cm.x, (cmt.x >> hs) & 0xffffu);
            outp[4u * k + 2u] = mix_nibble(w, half ? st.w : st.z, (stt.y >> hs) & 0xffffu, half ? cm.w : cm.z, (cmt.y >> hs) & 0xffffu);
        }
        __syncthreads();
        // pairs out: load-shaped again, 16 bytes = both nibbles of two positions per lane
#pragma unroll
        for (uint32_t i = 0; i < MW_XG; ++i) {
            const uint32_t j = i * MW_XS + xj, p = p0 + 2u * xq;
            const uint32_t slen = s0 + j < b.n_streams ? (b.in_sizes ? b.in_sizes[s0 + j] : b.stream_len) : 0u;
            if (p < slen)   // an odd stream's last quad carries one stale pair: it stays inside the (even) slot and is never read
                *(u32x4*)(b.sf + (size_t)(s0 + j) * b.sf_stride + 2u * p) = *(const u32x4*)(lds_out + j * MW_OUT_STRIDE + xq * 16u);
        }
        if (c + 1u < chunks) { MW_STAGE(buf ^ 1u) }
        __syncthreads();
    }
#undef MW_FETCH
#undef MW_STAGE
}

// The script interpreter of divans_gpu_selftest_cdf_ops_on (include/divans_gpu.h), implementation 2: the ops of
// cdf_ops_selftest_kernel (lit_kernels.hip) on the bucketed encoder's arithmetic.  The two rows are 8 packed dwords each in LDS
// and one lane walks them the way a lane of bucket_chain_kernel / mix_chain_kernel walks its bucket: bk_read, bk_pack, bk_add of
// the increment row from a table filled by bk_tab_entry (refilled when the script's speed changes), bk_renorm_at, store; the
// mixed step is mix_nibble on the records mix_chain_kernel's MX_POS forms.  The blend ops do not run bk_pack (ops 3 / 4 do), and op 2
// averages all 16 entries with average_rows + mix_total although production only ever averages entries sym and sym-1.  The encoder has no symbol search: op 4 finds the
// symbol with the reference's compare written out plainly and takes (start, freq) from bk_pack; op 9 is refused by the host.
__global__ __launch_bounds__(64) void cdf_ops_selftest_bucket_kernel(const u32x4* ops, uint32_t n, int32_t* out) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[2][8];
    __shared__ __attribute__((aligned(16))) uint32_t tab[128];
    const uint32_t lane = threadIdx.x;
    uint32_t tab_inc = 0u;
    for (uint32_t i = lane; i < 128u; i += 64u) tab[i] = bk_tab_entry(i, tab_inc);
    if (lane == 0u) bk_rows_reset(rows[0], 2u);
    __syncthreads();
    Weights w; w.w0 = 1; w.w1 = 1; w.norm = 1 << 14;
    for (uint32_t k = 0; k < n; ++k) {
        const u32x4 op = ops[k];
        const uint32_t kind = (uint32_t)__builtin_amdgcn_readfirstlane((int)op.x), sym = op.y & 15u;
        const bool is_blend = kind == 0u || kind == 1u || kind == 7u;
        if (is_blend && (uint32_t)__builtin_amdgcn_readfirstlane((int)op.z) != tab_inc) {
            tab_inc = (uint32_t)__builtin_amdgcn_readfirstlane((int)op.z);
            __syncthreads();
            for (uint32_t i = lane; i < 128u; i += 64u) tab[i] = bk_tab_entry(i, tab_inc);
            __syncthreads();
        }
        int32_t rec[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) rec[i] = 0;
        const uint16_t* r0 = (const uint16_t*)rows[0]; const uint16_t* r1 = (const uint16_t*)rows[1];
        if (kind == 5u) weights_update(w, (int)(short)op.y, (int)(short)op.z, (int)(short)op.w);
        if (kind == 6u) { w.w0 = 1; w.w1 = 1; w.norm = 1 << 14; }
        if (kind == 8u && op.y >= 2u) { if (op.z == 0u) w.w0 = (int)op.w; else if (op.z == 1u) w.w1 = (int)op.w; else w.norm = (int)(op.w & 0xffffu); }
        if (lane == 0u) {
            if (is_blend) {
                uint32_t* row = rows[kind == 1u];
                BkRow R = bk_read(row, tab, sym);
                bk_add(R);
                bk_renorm_at(R, (int)op.w);
                *(u32x4*)row = R.w0; *(u32x4*)(row + 4) = R.w1;
                for (int i = 0; i < 16; ++i) rec[i] = ((const uint16_t*)row)[i];
            } else if (kind == 2u) {
                const int cmax = r0[15], smax = r1[15];
                for (int i = 0; i < 15; ++i) rec[i] = average_rows(r0[i], r1[i], cmax, smax, (int)op.y);
                rec[15] = mix_total(cmax, smax);
            } else if (kind == 3u || kind == 4u) {
                uint32_t s = sym;
                if (kind == 4u) {       // probability/interface.rs:136-198: the first i < 15 with (slot * max >> 15) < cdf[i], else 15
                    const int rescaled = (int)(((op.y & 0x7fffu) * (uint32_t)r0[15]) >> 15);
                    s = 15u;
                    for (uint32_t i = 0; i < 15u; ++i) if (rescaled < (int)r0[i]) { s = i; break; }
                }
                const BkRow R = bk_read(rows[0], tab, s);
                const uint32_t sf = bk_pack(R, s);
                rec[0] = (int)(sf & 0xffffu); rec[1] = (int)(sf >> 16); rec[2] = (int)s;
            } else if (kind == 6u) {
                bk_rows_reset(rows[0], 2u);
                for (int i = 0; i < 16; ++i) rec[i] = r0[i];
            } else if (kind == 8u && op.y < 2u) {
                ((uint16_t*)rows[op.y])[op.z & 15u] = (uint16_t)op.w;
                for (int i = 0; i < 16; ++i) rec[i] = ((const uint16_t*)rows[op.y])[i];
            } else if (kind == 10u) {   // the records of MX_POS (entry sym | entry sym-1 << 16, the row totals), then mix_weights_kernel's step
                const BkRow C = bk_read(rows[0], tab, sym), S = bk_read(rows[1], tab, sym);
                const uint32_t cm_x = (uint32_t)C.chi | (sym ? (uint32_t)C.cprev << 16 : 0u), st_x = (uint32_t)S.chi | (sym ? (uint32_t)S.cprev << 16 : 0u);
                uint32_t mf = 0u;
                const uint32_t sf = mix_nibble<true>(w, st_x, S.w1.w >> 16, cm_x, C.w1.w >> 16, &mf);
                rec[0] = (int)(sf & 0xffffu); rec[1] = (int)(sf >> 16); rec[2] = (int)sym; rec[3] = (int)(mf & 0xffffu); rec[4] = (int)(mf >> 16);
                rec[5] = w.w0; rec[6] = w.w1; rec[7] = w.norm;
            }
            if (kind == 5u || (kind == 8u && op.y >= 2u)) { rec[0] = w.w0; rec[1] = w.w1; rec[2] = w.norm; }
#pragma unroll
            for (int i = 0; i < 16; ++i) out[(size_t)k * 16u + (uint32_t)i] = rec[i];
        }
        if (kind == 10u) {              // lane 0 ran the update: every lane keeps the same Weights
            w.w0 = __builtin_amdgcn_readfirstlane(w.w0); w.w1 = __builtin_amdgcn_readfirstlane(w.w1); w.norm = __builtin_amdgcn_readfirstlane(w.norm);
        }
    }
}

hipError_t launch_selftest_cdf_ops_bucket(const uint32_t* d_ops, uint32_t n, int32_t* d_out, hipStream_t st) {
    hipLaunchKernelGGL(cdf_ops_selftest_bucket_kernel, dim3(1), dim3(64), 0, st, (const u32x4*)d_ops, n, d_out);
    return hipGetLastError();
}

// defined behind launch_bucket_mix_model: the SEG instances are then instantiated behind every other kernel of the file, and the
// kernels of the default path keep their places in the code object
static void launch_mix_sort_seg(int model, const MixBucketBatch& b, hipStream_t st);

hipError_t launch_bucket_mix_model(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st) {
    BucketBatch v;                       // the view the shared task-list and unsort kernels take
    v.in = b.in; v.in_offsets = b.in_offsets; v.in_sizes = b.in_sizes;
    v.n_streams = b.n_streams; v.stream_len = b.stream_len; v.max_stream_len = b.max_stream_len; v.pieces = b.pieces;
    v.slot = b.slot; v.sf_stride = 2u * b.pos_stride;   // pos_stride == slot: the unsort below is in place
    v.sorted = nullptr; v.inv = b.inv; v.desc = b.desc; v.sfs = nullptr; v.sf = nullptr; v.tasks = b.tasks; v.counters = b.counters;
    v.inc = 0; v.lim = 0;
    v.seg_begin = nullptr; v.segs = nullptr; v.bt_first = 0; v.n_btypes = 0; v.status = nullptr;   // (the sort kernels here take `b`)
    for (int model = 0; model < 2; ++model) {
        hipError_t e = hipMemsetAsync(b.counters, 0, 64, st);
        if (e != hipSuccess) return e;
        if (b.pieces < 8u) {
            e = hipMemsetAsync(b.desc, 0, (size_t)b.n_streams * 256u * 8u * sizeof(uint32_t), st);
            if (e != hipSuccess) return e;
        }
        if (model == 0) {
            if (b.segs) launch_mix_sort_seg(0, b, st);
            else hipLaunchKernelGGL((mix_sort_kernel<0, false>), dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
            launch_bucket_tasks(v, st);
            hipLaunchKernelGGL(mix_chain_kernel<0>, dim3(num_cus * MX_CHAIN_WAVES), dim3(64), MxGeom<0>::LDS_BYTES, st, b);
        } else {
            if (b.segs) launch_mix_sort_seg(1, b, st);
            else hipLaunchKernelGGL((mix_sort_kernel<1, false>), dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
            launch_bucket_tasks(v, st);
            hipLaunchKernelGGL(mix_chain_kernel<1>, dim3(num_cus * MX_CHAIN_WAVES), dim3(64), MxGeom<1>::LDS_BYTES, st, b);
        }
        v.sfs = b.xs[model]; v.sf = (uint32_t*)b.xs[model]; v.sf_stride = 2u * b.pos_stride;
        launch_bucket_unsort(v, st);
        v.sfs = (bk_u32x2*)b.maxes[model]; v.sf = b.maxes[model]; v.sf_stride = b.pos_stride;
        launch_bucket_unsort32(v, st);
    }
    if ((b.n_streams + 31u) / 32u > num_cus * 4u) hipLaunchKernelGGL(mix_weights_kernel<2>, dim3((b.n_streams + 31u) / 32u), dim3(64), 0, st, b);
    else hipLaunchKernelGGL(mix_weights_kernel<1>, dim3((b.n_streams + 31u) / 32u), dim3(64), 0, st, b);
    return hipGetLastError();
}

static void launch_mix_sort_seg(int model, const MixBucketBatch& b, hipStream_t st) {
    if (model == 0) hipLaunchKernelGGL((mix_sort_kernel<0, true>), dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
    else hipLaunchKernelGGL((mix_sort_kernel<1, true>), dim3(b.n_streams * b.pieces), dim3(BK_SORT_THREADS), 0, st, b);
}

// ---------------------------------------------------------------------------------------------
// The context-keyed pass (lit_bucket_ctx.hip: every mixing value 0).  Both models' rows are keyed by ctx, so both chain launches
// walk the buckets of ONE sort with the geometry of the context model (1 high row + 16 low rows):
//   model 0   high[0][0][ctx], low[0][ctx][hi], both blended with literal_adaptation[0] (literal.rs:320,354), into xs[0] / maxes[0]:
//             MxChain<1> with the other planes, and the kernel below with the other speeds
//   model 1   First[ctx], Second[hi][ctx]: mix_chain_kernel<1> as it is
// The kernel is a template (PLANE = the record planes it fills; 0 is the one instance) so that it is emitted where
// launch_mix_chain_ctx names it -- behind every other kernel of the file, as the SEG sorts are.
// ---------------------------------------------------------------------------------------------
template <int PLANE> struct MxChainCtx : MxChain<1> {
    static __device__ __forceinline__ Slot slot(const MixBucketBatch& b, size_t off) { return {b.xs[PLANE] + off, b.maxes[PLANE] + off}; }
};

template <int PLANE>
__global__ __launch_bounds__(64) void mix_chain_ctx_kernel(const MixBucketBatch b) {
    using G = MxGeom<1>;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
    const uint32_t lane = threadIdx.x;
    uint32_t* my = lds32 + lane * G::LANE_DW;
    uint32_t* tabh = lds32 + 64u * G::LANE_DW;
    uint32_t* tabl = tabh + 128u;
    for (uint32_t i = lane; i < 128u; i += 64u) {
        tabh[i] = bk_tab_entry(i, (uint32_t)b.inc0);
        tabl[i] = tabh[i];
    }
    __syncthreads();
    const typename MxChainCtx<PLANE>::Env env = {my, tabh, tabl, b.lim0, b.lim0};
    bk_chain_loop<MxChainCtx<PLANE>>(env, b);
}

void launch_mix_chain_ctx(const MixBucketBatch& b, int model, uint32_t num_cus, hipStream_t st) {
    if (model == 0) hipLaunchKernelGGL(mix_chain_ctx_kernel<0>, dim3(num_cus * MX_CHAIN_WAVES), dim3(64), MxGeom<1>::LDS_BYTES, st, b);
    else hipLaunchKernelGGL(mix_chain_kernel<1>, dim3(num_cus * MX_CHAIN_WAVES), dim3(64), MxGeom<1>::LDS_BYTES, st, b);
}

// the choice launch_bucket_mix_model makes (which keeps its own text: the instances stay where they are in the code object)
void launch_mix_weights(const MixBucketBatch& b, uint32_t num_cus, hipStream_t st) {
    if ((b.n_streams + 31u) / 32u > num_cus * 4u) hipLaunchKernelGGL(mix_weights_kernel<2>, dim3((b.n_streams + 31u) / 32u), dim3(64), 0, st, b);
    else hipLaunchKernelGGL(mix_weights_kernel<1>, dim3((b.n_streams + 31u) / 32u), dim3(64), 0, st, b);
}

// the chain launches of launch_bucket_mix_model, for the pass that brings its own sorts (launch_bucket_mix_bt_model, lit_bucket_ctx.hip)
void launch_mix_chain(const MixBucketBatch& b, int model, uint32_t num_cus, hipStream_t st) {
    if (model == 0) hipLaunchKernelGGL(mix_chain_kernel<0>, dim3(num_cus * MX_CHAIN_WAVES), dim3(64), MxGeom<0>::LDS_BYTES, st, b);
    else hipLaunchKernelGGL(mix_chain_kernel<1>, dim3(num_cus * MX_CHAIN_WAVES), dim3(64), MxGeom<1>::LDS_BYTES, st, b);
}

}  // namespace divans_hip
