// lit_commands.hip -- general streams ENCODED from their command lists (divans_gpu_lit_encode_commands_batch): the step in front of
// the segment encoders.  A compressor has the raw bytes and the Literal / Copy / Insert list its match finder wrote; the encoders want
// the literal bytes in command order and one LitSegment {len, btype, last8} per Literal command.  This kernel derives the one from
// the other -- walk() of ir.cpp on the device -- and checks on the way that the list describes the raw bytes: status 0 means the
// decoder, given the same list, produces them again.
//
// Nothing here is serial per byte.  A stream's commands tile its raw range, so a command's raw position, literal position and segment
// index are exclusive prefix sums over the list, and every byte a Copy refers to already exists in the raw buffer: no store is read
// back, nothing is drained, plain loads and stores throughout.
//
// One wave per stream, 64 commands (one per lane) per block:
//   1. check the kinds, scan len / literal len / "a Literal command with bytes" across the wave (64-bit sums: lengths up to 2^32 - 1
//      cannot wrap a position), carry the sums from block to block;
//   2. check every command of the block against the raw size, the bytes produced so far, the insert size, the block-type count and
//      lit_stream_len BEFORE any byte of the block is read; the first command that fails names the stream's status bit and ends the walk;
//   3. lanes holding a Literal command with bytes write its segment (last8 = the eight bytes in front of it in history ++ raw);
//   4. the wave walks the block's contiguous raw range, PIECE bytes per lane and step.  A lane finds the command that covers its piece
//      in the block's start positions (LDS, binary search); a piece inside one command moves or compares as a whole, one that crosses
//      command boundaries goes byte by byte with the command index running along.  Literals go to the stream's literal slot, COPY bytes
//      are compared with raw[p - distance], INSERT bytes with the insert bytes.
// History (divans_gpu_lit_encode_commands_history_batch): hist_sizes[s] known bytes lie logically in front of raw[0].  A distance may
// then reach pos + hlen, last8 of a Literal command near the stream's start takes the history's tail, and a COPY piece is compared
// with history where p - distance < 0: as a whole when it lies wholly there, byte by byte when its source straddles the history's end.
// History is only read and may lie inside the raw buffer itself (the pieces of one file, each with the bytes in front of it).
// Segment begins: exact.  lit_commands_count_kernel counts every stream's Literal commands with bytes, lit_commands_scan_kernel turns
// the counts into seg_begin[0 .. n_streams] (an exclusive sum, saturated at the records the host allocated: one per command), and the
// prepare kernel writes stream s's segments at segs[seg_begin[s] ..].  (One slot per command with the tail filled with empty
// segments needs no counting pass, but the streaming encoders walk a list's trailing empty segments one load at a time: measured, that
// cost more than the prepare step itself.)  A stream that fails gets empty segments {0, bt_first, 0} only -- the segment contract
// allows them, they code nothing -- and literal size 0: it is coded as a stream without literals.
#include "lit_kernels.h"

namespace divans_hip {

constexpr uint32_t CMDS_THREADS = 256;      // four waves = four streams per workgroup; the waves never meet
constexpr uint32_t CMDS_BLOCK = 64;         // commands per block: one per lane
constexpr uint32_t CMDS_PIECE = 16;         // raw bytes per lane and step of the data walk

typedef unsigned int cm_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t cmds_wave_scan(uint64_t v, uint32_t lane) {     // inclusive
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
        if (lane >= d) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ uint64_t cmds_wave_last(uint64_t v) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, 63, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), 63, 64);
    return ((uint64_t)hi << 32) | lo;
}
// the lanes of a wave exchange values through LDS: what was written is visible to every lane behind this
__device__ __forceinline__ void cmds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct CmdPieces { uint8_t v[CMDS_PIECE]; };
__device__ __forceinline__ CmdPieces cmds_load_piece(const uint8_t* p) { CmdPieces r; __builtin_memcpy(r.v, p, CMDS_PIECE); return r; }
__device__ __forceinline__ bool cmds_same(const CmdPieces& a, const CmdPieces& b) {
    cm_u32x4 x, y;
    __builtin_memcpy(&x, a.v, 16); __builtin_memcpy(&y, b.v, 16);
    return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) == 0u;
}

// The byte a COPY of distance `arg` repeats at raw position q: (history ++ raw)[q - arg].  The command was checked: arg - q <= hlen.
__device__ __forceinline__ uint8_t cmds_copy_source(const uint8_t* raw, const uint8_t* hist, uint32_t hlen, uint32_t q, uint32_t arg) {
    return q >= arg ? raw[q - arg] : hist[hlen - (arg - q)];
}

// the stream's commands [c0, c1): begins that do not ascend, or that leave what the host read as the batch's ends, give no list
__device__ __forceinline__ bool cmds_range(const LitCommandPrepare& b, uint32_t s, uint32_t& c0, uint32_t& c1) {
    c0 = b.cmd_begin[s]; c1 = b.cmd_begin[s + 1u];
    if (c0 >= b.cmd_first && c1 >= c0 && c1 <= b.cmd_last) return true;
    c0 = c1 = b.cmd_first;
    return false;
}

// seg_begin[1 + s] = the Literal commands with bytes of stream s (whatever else is wrong with the list: the prepare kernel fills what
// it does not use with empty segments)
__global__ __launch_bounds__(CMDS_THREADS) void lit_commands_count_kernel(const LitCommandPrepare b) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * (CMDS_THREADS / 64u) + (threadIdx.x >> 6);
    if (s >= b.n_streams) return;
    uint32_t c0, c1;
    cmds_range(b, s, c0, c1);
    uint32_t mine = 0u;
    for (uint32_t i = c0 + lane; i < c1; i += 64u) {
        const LitCommand c = b.cmds[i];
        mine += (c.kind == LIT_CMD_LITERAL && c.len != 0u) ? 1u : 0u;
    }
    for (uint32_t d = 32u; d != 0u; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, (int)d, 64);
    if (lane == 0u) b.seg_begin[1u + s] = mine;
}

// seg_begin[s] = the counts in front of stream s, saturated at the records `segs` holds (ascending begins never reach it: a stream
// has at most one segment per command); one workgroup
__global__ __launch_bounds__(1024) void lit_commands_scan_kernel(const LitCommandPrepare b) {
    __shared__ uint64_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint64_t cap = b.cmd_last - b.cmd_first;
    uint64_t run = 0u;
    if (tid == 0u) b.seg_begin[0] = 0u;
    for (uint32_t s0 = 0; s0 < b.n_streams; s0 += 1024u) {       // workgroup-uniform
        const uint32_t s = s0 + tid;
        const uint64_t v = s < b.n_streams ? b.seg_begin[1u + s] : 0u;
        const uint64_t incl = cmds_wave_scan(v, lane);
        if (lane == 63u) wsum[w] = incl;
        __syncthreads();
        uint64_t before = run, all = 0u;
        for (uint32_t j = 0; j < 16u; ++j) { if (j < w) before += wsum[j]; all += wsum[j]; }
        __syncthreads();
        const uint64_t end = before + incl;
        if (s < b.n_streams) b.seg_begin[1u + s] = (uint32_t)(end < cap ? end : cap);
        run += all;
    }
}

// HIST: the streams have history.  A compile-time choice, as in the decoder's CmdCursor: as a branch at run time it cost lists
// without history 2 % of the prepare step (profiles/r17_command_history_rate.txt); a call without history runs the kernel it ran before.
template <bool HIST>
__device__ __forceinline__ void commands_prepare_body(const LitCommandPrepare& b) {
    // per wave: the block's raw start positions (one more: the block's end), kinds, arguments and literal positions
    __shared__ uint32_t s_start[CMDS_THREADS / 64u][CMDS_BLOCK + 1u];
    __shared__ uint32_t s_kind[CMDS_THREADS / 64u][CMDS_BLOCK], s_arg[CMDS_THREADS / 64u][CMDS_BLOCK], s_lit[CMDS_THREADS / 64u][CMDS_BLOCK];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * (CMDS_THREADS / 64u) + w;
    if (s >= b.n_streams) return;
    const uint8_t* raw = b.raw + b.raw_offsets[s];
    const uint64_t raw_size = b.raw_sizes[s];
    const uint8_t* ins = b.ins ? b.ins + b.ins_offsets[s] : nullptr;
    const uint32_t ins_size = b.ins ? b.ins_sizes[s] : 0u;
    const uint8_t* hist = HIST && b.hist ? b.hist + b.hist_offsets[s] : nullptr;     // the bytes logically in front of raw[0] (may lie inside b.raw)
    const uint32_t hlen = HIST && b.hist ? b.hist_sizes[s] : 0u;
    uint8_t* lit = b.lit + (uint64_t)s * b.lit_slot;
    uint32_t c0, c1;
    uint32_t flags = cmds_range(b, s, c0, c1) ? 0u : LIT_STATUS_BAD_COMMAND;
    // the stream's segment records: as many as it has Literal commands with bytes (fewer only where begins that do not ascend made
    // the scan saturate: such a list fails below)
    const uint32_t seg0 = b.seg_begin[s], seg_room = b.seg_begin[s + 1u] - seg0;
    LitSegment* segs = b.segs + seg0;
    uint64_t pos = 0u, lpos = 0u;       // raw bytes, literal bytes in front of the block
    uint32_t nseg = 0u;                 // segments written so far
    bool differs = false;               // this lane met a COPY / INSERT byte that is not the raw byte at its place
    for (uint32_t i0 = c0; i0 < c1 && !flags; i0 += CMDS_BLOCK) {
        const uint32_t i = i0 + lane;
        LitCommand c = {LIT_CMD_COPY, 0u, 0u, 0u};      // behind the list: a command that does nothing
        if (i < c1) c = b.cmds[i];
        const bool known = c.kind == LIT_CMD_COPY || c.kind == LIT_CMD_INSERT || c.kind == LIT_CMD_LITERAL;
        const bool is_lit = c.kind == LIT_CMD_LITERAL;
        const uint64_t e_all = cmds_wave_scan(c.len, lane), e_lit = cmds_wave_scan(is_lit ? c.len : 0u, lane);
        const bool is_seg = is_lit && c.len != 0u;
        const uint32_t e_seg = (uint32_t)cmds_wave_scan(is_seg ? 1u : 0u, lane);
        const uint64_t start = pos + e_all - c.len, lstart = lpos + e_lit - (is_lit ? c.len : 0u);
        // the verdict of this command, in the decoder's order (a command of length 0 is checked for its kind alone)
        uint32_t verdict = 0u;
        if (!known) verdict = LIT_STATUS_BAD_COMMAND;
        else if (c.len != 0u) {
            if (start + c.len > raw_size) verdict = LIT_STATUS_BAD_COMMAND;
            else if (is_lit) {
                if (c.arg - b.bt_first >= b.n_btypes || lstart + c.len > b.lit_stream_len) verdict = LIT_STATUS_BAD_SEGMENT;
            } else if (c.kind == LIT_CMD_COPY) {
                if (c.arg == 0u || (c.arg > start && (!HIST || c.arg - start > hlen))) verdict = LIT_STATUS_BAD_COMMAND;
            } else if (c.arg > ins_size || c.len > ins_size - c.arg) verdict = LIT_STATUS_BAD_COMMAND;
        }
        if (nseg + (uint32_t)__shfl((int)e_seg, 63, 64) > seg_room) verdict = LIT_STATUS_BAD_COMMAND;     // (uniform)
        const unsigned long long failed = __ballot(verdict != 0u);
        if (failed) {       // the first command that cannot run decides, as it does in the decoder; nothing of the block is touched
            flags = (uint32_t)__shfl((int)verdict, __ffsll((long long)failed) - 1, 64);
            break;
        }
        // from here on every position of the block lies inside the raw size: 32 bits hold it
        if (is_seg) {
            uint64_t l8 = 0u;
            if (start >= 8u) __builtin_memcpy(&l8, raw + start - 8u, 8);
            else if (!HIST) for (uint32_t k = 0; k < (uint32_t)start; ++k) l8 |= (uint64_t)raw[k] << (8u * (8u - (uint32_t)start + k));
            else for (uint32_t k = 0; k < 8u; ++k) {     // byte k of last8 = history ++ raw at start - 8 + k, zero in front of the history
                const uint32_t t = (uint32_t)start + k;
                uint32_t v = 0u;
                if (t >= 8u) v = raw[t - 8u];
                else if (hlen >= 8u - t) v = hist[hlen - (8u - t)];
                l8 |= (uint64_t)v << (8u * k);
            }
            const LitSegment sg = {c.len, c.arg, (uint32_t)l8, (uint32_t)(l8 >> 32)};
            segs[nseg + e_seg - 1u] = sg;
        }
        cmds_wave_sync();       // the walk of the block before is done with the arrays
        s_start[w][lane] = (uint32_t)start; s_kind[w][lane] = c.kind; s_arg[w][lane] = c.arg; s_lit[w][lane] = (uint32_t)lstart;
        const uint64_t blk_end = cmds_wave_last(pos + e_all);
        if (lane == 0u) s_start[w][CMDS_BLOCK] = (uint32_t)blk_end;
        cmds_wave_sync();
        const uint32_t* st = s_start[w];
        for (uint64_t p0 = pos + (uint64_t)lane * CMDS_PIECE; p0 < blk_end; p0 += 64u * CMDS_PIECE) {
            // the last command that starts at or in front of p0: it has bytes (the empty ones in front of it start there too)
            uint32_t j = 0u;
#pragma unroll
            for (uint32_t step = CMDS_BLOCK / 2u; step != 0u; step >>= 1) if (st[j + step] <= (uint32_t)p0) j += step;
            const uint32_t p = (uint32_t)p0;
            if (p0 + CMDS_PIECE <= (uint64_t)st[j + 1u]) {        // the piece lies inside command j (and so inside the block)
                const uint32_t kind = s_kind[w][j], arg = s_arg[w][j], off = p - st[j];
                const CmdPieces v = cmds_load_piece(raw + p);
                if (kind == LIT_CMD_LITERAL) __builtin_memcpy(lit + s_lit[w][j] + off, v.v, CMDS_PIECE);
                else if (kind == LIT_CMD_COPY) {
                    if (!HIST || arg <= p) differs |= !cmds_same(v, cmds_load_piece(raw + p - arg));
                    else if (arg - p >= CMDS_PIECE) differs |= !cmds_same(v, cmds_load_piece(hist + (hlen - (arg - p))));      // wholly history
                    else for (uint32_t k = 0; k < CMDS_PIECE; ++k) differs |= v.v[k] != cmds_copy_source(raw, hist, hlen, p + k, arg);
                }
                else differs |= !cmds_same(v, cmds_load_piece(ins + arg + off));
            } else {
                const uint32_t n = blk_end - p0 < CMDS_PIECE ? (uint32_t)(blk_end - p0) : CMDS_PIECE;
                for (uint32_t k = 0; k < n; ++k) {
                    const uint32_t q = p + k;
                    while (st[j + 1u] <= q) ++j;        // st[CMDS_BLOCK] = the block's end > q
                    const uint32_t kind = s_kind[w][j], arg = s_arg[w][j], off = q - st[j];
                    const uint8_t v = raw[q];
                    if (kind == LIT_CMD_LITERAL) lit[s_lit[w][j] + off] = v;
                    else if (kind == LIT_CMD_COPY) differs |= v != (HIST ? cmds_copy_source(raw, hist, hlen, q, arg) : raw[q - arg]);
                    else differs |= v != ins[arg + off];
                }
            }
        }
        pos = blk_end; lpos = cmds_wave_last(lpos + e_lit); nseg += (uint32_t)__shfl((int)e_seg, 63, 64);
    }
    if (!flags && (__ballot(differs) != 0ull || pos != raw_size)) flags = LIT_STATUS_BAD_COMMAND;
    // after a fault all of the stream's segment records are empty segments
    const LitSegment none = {0u, b.bt_first, 0u, 0u};
    for (uint32_t k = (flags ? 0u : nseg) + lane; k < seg_room; k += 64u) segs[k] = none;
    if (lane == 0u) {
        const uint32_t n_lit = flags ? 0u : (uint32_t)lpos;
        b.lit_sizes[s] = n_lit; b.out_lit_sizes[s] = n_lit;
        b.lit_offsets[s] = (uint64_t)s * b.lit_slot;
        if (flags) {
            if (b.status) atomicOr(b.status, flags);
            if (b.stream_bad) b.stream_bad[s] = 1;
        }
    }
}

__global__ __launch_bounds__(CMDS_THREADS) void lit_commands_prepare_kernel(const LitCommandPrepare b) { commands_prepare_body<false>(b); }
__global__ __launch_bounds__(CMDS_THREADS) void lit_commands_prepare_history_kernel(const LitCommandPrepare b) { commands_prepare_body<true>(b); }

hipError_t launch_commands_prepare(const LitCommandPrepare& b, hipStream_t st) {
    const uint32_t per = CMDS_THREADS / 64u;
    hipLaunchKernelGGL(lit_commands_count_kernel, dim3((b.n_streams + per - 1u) / per), dim3(CMDS_THREADS), 0, st, b);
    hipLaunchKernelGGL(lit_commands_scan_kernel, dim3(1), dim3(1024), 0, st, b);
    if (b.hist) hipLaunchKernelGGL(lit_commands_prepare_history_kernel, dim3((b.n_streams + per - 1u) / per), dim3(CMDS_THREADS), 0, st, b);
    else hipLaunchKernelGGL(lit_commands_prepare_kernel, dim3((b.n_streams + per - 1u) / per), dim3(CMDS_THREADS), 0, st, b);
    return hipGetLastError();
}

}  // namespace divans_hip
