// TEST HARNESS: the decode kernels' own source on the CPU, driven through the batch C ABI (tests/c/README.md, "Device code on the CPU").
// divans_amd/csrc/capi.cpp chooses instance, grid, LDS, cache organisation and tables as it does on a GPU; the launches of
// lit_decode2.hip -- compiled for the host against tests/c/simt -- run lane by lane inside this process, on the memory of
// tests/c/fakehip_rt.cpp.  Everything is built with -fsanitize=address,undefined; nothing is preloaded.
//
//   device_code CASES.bin POISON            every case of the file with fresh LDS and fresh device memory holding the byte POISON
//   device_code work WORK.bin POISON        the work-array shape (below) from the streams the file lists
// The test module runs one process per poison byte side by side and compares their RAN lines: a difference is a read of memory
// nobody wrote.
//
// A case is one batch of coded streams (the oracle's bytes) with the raw bytes they must decode to, and a list of decoder settings
// applied one after the other to one codec, as tests/test_gpu_plain_decoders.py does.  Per run the program prints
//   RAN <case> | <setting> | <kernel the library names> | status <word> | grid <workgroups> | out <hash of the whole output buffer>
// and at the end one "SIMT RAN <instance>" line per kernel instance the stand-in executed.  A wrong byte, a status other than the
// case's or a kernel the stand-in did not run under the library's name ends it
// with "EXPECTATION FAILED"; an access outside LDS or a buffer resource with "SIMT FINDING"; anything else is the sanitizers'.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "divans_gpu.h"
#include "fakehip_rt.h"
#include "simt/simt_driver.h"

#define FAIL(...) do { fprintf(stderr, "EXPECTATION FAILED [%s]: ", g_label.c_str()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(1); } while (0)
#define OK(call) do { const int rc_ = (call); if (rc_ != 0) FAIL("%s -> %d (%s)", #call, rc_, divans_gpu_last_error()); } while (0)
#define HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) FAIL("%s -> %d", #call, (int)e_); } while (0)

static std::string g_label = "start";

struct Reader {
    std::vector<uint8_t> data; size_t at = 0;
    void need(size_t n) { if (at + n > data.size()) { fprintf(stderr, "case file truncated at byte %zu\n", at); exit(2); } }
    uint32_t u32() { need(4); uint32_t v; memcpy(&v, &data[at], 4); at += 4; return v; }
    uint64_t u64() { need(8); uint64_t v; memcpy(&v, &data[at], 8); at += 8; return v; }
    std::vector<uint8_t> bytes(size_t n) { need(n); std::vector<uint8_t> v(data.begin() + at, data.begin() + at + n); at += n; return v; }
    std::string str() { const uint32_t n = u32(); const std::vector<uint8_t> b = bytes(n); return std::string(b.begin(), b.end()); }
    template <class T> std::vector<T> array(size_t n) { const std::vector<uint8_t> b = bytes(n * sizeof(T)); std::vector<T> v(n); if (n) memcpy(v.data(), b.data(), b.size()); return v; }
};

struct Setting { uint32_t generation, rows[4], shifts[4], blocks, pinning; std::string label; };
struct Case {
    std::string name;
    divans_lit_config cfg;
    uint32_t set_types, max_stream_len, n, longest, has_segs, expect_status;
    std::vector<uint8_t> coded; std::vector<uint64_t> coff; std::vector<uint32_t> csz;
    std::vector<uint8_t> expect, blank; std::vector<uint64_t> ooff; std::vector<uint32_t> osz;
    std::vector<uint32_t> seg_begin; std::vector<divans_lit_segment> segs;
    std::vector<Setting> settings;
};

static std::vector<Case> read_cases(const char* path) {
    Reader r;
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) r.data.insert(r.data.end(), buf, buf + k);
    fclose(f);
    if (r.bytes(8) != std::vector<uint8_t>{'D', 'V', 'S', 'I', 'M', 'T', '0', '1'}) { fprintf(stderr, "%s is no case file\n", path); exit(2); }
    std::vector<Case> cases(r.u32());
    for (Case& c : cases) {
        c.name = r.str();
        const std::vector<uint8_t> cfg = r.bytes(sizeof(divans_lit_config));
        memcpy(&c.cfg, cfg.data(), cfg.size());
        c.set_types = r.u32(); c.max_stream_len = r.u32(); c.n = r.u32(); c.longest = r.u32(); c.has_segs = r.u32(); c.expect_status = r.u32();
        c.coded = r.bytes(r.u64()); c.coff = r.array<uint64_t>(c.n); c.csz = r.array<uint32_t>(c.n);
        const uint64_t out_len = r.u64();
        c.expect = r.bytes(out_len); c.blank = r.bytes(out_len); c.ooff = r.array<uint64_t>(c.n); c.osz = r.array<uint32_t>(c.n);
        if (c.has_segs) { c.seg_begin = r.array<uint32_t>(c.n + 1); c.segs = r.array<divans_lit_segment>(r.u32()); }
        c.settings.resize(r.u32());
        for (Setting& s : c.settings) {
            s.generation = r.u32();
            for (uint32_t& v : s.rows) v = r.u32();
            for (uint32_t& v : s.shifts) v = r.u32();
            s.blocks = r.u32(); s.pinning = r.u32(); s.label = r.str();
        }
    }
    if (r.at != r.data.size()) { fprintf(stderr, "%zu bytes behind the last case\n", r.data.size() - r.at); exit(2); }
    return cases;
}

// an exact-size device block holding `v` (one byte where it is empty: hipMalloc(0) gives no pointer)
template <class T> static T* dev(const std::vector<T>& v, std::vector<void*>& mine) {
    void* p = nullptr;
    HIP(hipMalloc(&p, v.empty() ? 1 : v.size() * sizeof(T)));
    if (!v.empty()) HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    mine.push_back(p);
    return (T*)p;
}

struct Batch {      // what one decode call is given and what it must leave
    uint32_t n, longest; bool segs;
    const uint8_t* d_coded; const uint64_t* d_coff; const uint32_t* d_csz;
    const uint32_t* d_seg_begin; const divans_lit_segment* d_segs;
    uint8_t* d_out; const uint64_t* d_ooff; const uint32_t* d_osz;
    const std::vector<uint8_t>* expect; const std::vector<uint64_t>* ooff; const std::vector<uint32_t>* osz;
    uint32_t expect_status;
};

// one decode call of the batch C ABI: prints the RAN line, then every byte of the output buffer, the status word, the instance
static void call_and_check(divans_gpu_codec* codec, const Batch& b) {
    const std::vector<std::pair<std::string, uint64_t>> ran_before = simt::instances();
    const size_t launches_before = fakehip::launches().size();
    if (b.segs) OK(divans_gpu_lit_decode_segments_batch(codec, b.d_coded, b.d_coff, b.d_csz, b.n, b.d_seg_begin, b.d_segs, b.d_out, b.d_ooff, b.d_osz, b.longest));
    else OK(divans_gpu_lit_decode_batch(codec, b.d_coded, b.d_coff, b.d_csz, b.n, b.d_out, b.d_ooff, b.d_osz, b.longest));
    // a launch that reached the recording runtime is a kernel of a host-only file: it did NOT run
    for (size_t i = launches_before; i < fakehip::launches().size(); ++i) FAIL("%s was launched and is not compiled for the stand-in: the call's result would miss its work", fakehip::launches()[i].kernel.c_str());
    uint32_t status = 0;
    OK(divans_gpu_codec_status(codec, &status));
    char name[200];
    OK(divans_gpu_codec_last_decode_kernel(codec, name, sizeof name));
    uint64_t before = 0;
    for (const auto& kv : ran_before) if (kv.first == name) before = kv.second;
    std::vector<uint8_t> out(b.expect->size());
    if (!out.empty()) HIP(hipMemcpy(out.data(), b.d_out, out.size(), hipMemcpyDeviceToHost));
    uint64_t h = 1469598103934665603ull;       // FNV-1a of the whole output buffer: two runs under different poison bytes are compared by it
    for (uint8_t v : out) h = (h ^ v) * 1099511628211ull;
    if (simt::launches_of(name) != before + 1) FAIL("the library names %s: the stand-in ran it %llu times during the call", name, (unsigned long long)(simt::launches_of(name) - before));
    printf("RAN %s | %s | status %u | grid %u | out %016llx\n", g_label.c_str(), name, status, simt::last_grid(name), (unsigned long long)h);
    fflush(stdout);
    for (size_t i = 0; i < out.size(); ++i) {
        if (out[i] == (*b.expect)[i]) continue;
        for (uint32_t k = 0; k < b.n; ++k) if (i >= (*b.ooff)[k] && i < (*b.ooff)[k] + (*b.osz)[k]) FAIL("stream %u (%u bytes) decoded wrong from its byte %zu: 0x%02x for 0x%02x (%s)", k, (*b.osz)[k], i - (size_t)(*b.ooff)[k], out[i], (*b.expect)[i], name);
        FAIL("sentinel byte %zu of the output written to (%s)", i, name);
    }
    if (status != b.expect_status) FAIL("status %u, expected %u (%s)", status, b.expect_status, name);
}

static void run_case(const Case& c) {
    std::vector<void*> mine;
    divans_gpu_codec* codec = nullptr;
    g_label = c.name;
    OK(divans_gpu_codec_create(&codec, &c.cfg, 0, nullptr, c.max_stream_len));
    if (c.set_types) OK(divans_gpu_codec_set_block_types(codec, c.set_types));
    Batch b;
    b.n = c.n; b.longest = c.longest; b.segs = c.has_segs != 0; b.expect = &c.expect; b.ooff = &c.ooff; b.osz = &c.osz; b.expect_status = c.expect_status;
    b.d_coded = dev(c.coded, mine); b.d_coff = dev(c.coff, mine); b.d_csz = dev(c.csz, mine);
    b.d_ooff = dev(c.ooff, mine); b.d_osz = dev(c.osz, mine);
    b.d_seg_begin = c.has_segs ? dev(c.seg_begin, mine) : nullptr;
    b.d_segs = c.has_segs ? dev(c.segs, mine) : nullptr;
    for (const Setting& s : c.settings) {
        g_label = c.name + " | " + s.label;
        fakehip::set_case(g_label.c_str());
        if (s.pinning != ~0u) OK(divans_gpu_codec_set_high_row_pinning(codec, s.pinning));
        if (s.generation) OK(divans_gpu_codec_set_decoder(codec, s.generation, s.rows[0] == ~0u ? nullptr : s.rows, s.rows[0] == ~0u ? nullptr : s.shifts, s.blocks));
        else if (s.blocks) OK(divans_gpu_codec_set_geometry(codec, s.blocks, ~0u));
        b.d_out = dev(c.blank, mine);
        call_and_check(codec, b);
    }
    divans_gpu_codec_destroy(codec);
    for (void* p : mine) HIP(hipFree(p));
}

// ---- the work-array shape (tests/test_gpu_far_offsets.py, test_work_arrays_past_4g; DESIGN.md section 4, the first occurrence of the
// open m6 fault): n_streams streams on a codec for max_stream_len-byte streams, the literals back to back, the coded bytes
// right-aligned in slots of divans_gpu_lit_encode_bound(max_stream_len) -- gigabytes of slots on the runtime's lazily committed pages,
// 64-bit offsets past 2^32 --, a natural two-segment list a stream, decode_batch and then decode_segments_batch on ONE codec with the
// library's own launch.  The file lists the streams that have bytes (the threshold form: the ones around every threshold of
// far_offset_cases.THRESHOLDS; the full form: all of them); every other stream has length 0.  The coded bytes are the oracle's.
static void run_work(const char* path) {
    Reader r;
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) r.data.insert(r.data.end(), buf, buf + k);
    fclose(f);
    if (r.bytes(8) != std::vector<uint8_t>{'D', 'V', 'W', 'O', 'R', 'K', '0', '1'}) { fprintf(stderr, "%s is no work file\n", path); exit(2); }
    const std::string name = r.str();
    divans_lit_config cfg;
    { const std::vector<uint8_t> b = r.bytes(sizeof cfg); memcpy(&cfg, b.data(), b.size()); }
    const uint32_t set_types = r.u32(), msl = r.u32(), n = r.u32(), listed = r.u32();
    std::vector<uint32_t> osz(n, 0), csz(n, 0), seg_begin(n + 1);
    std::vector<uint64_t> ooff(n), coff(n);
    std::vector<divans_lit_segment> segs(2 * (size_t)n);
    memset(segs.data(), 0, segs.size() * sizeof(segs[0]));
    struct Listed { uint32_t index; std::vector<uint8_t> lit, coded; uint64_t last8; };
    std::vector<Listed> streams(listed);
    for (Listed& s : streams) {
        s.index = r.u32(); s.last8 = r.u64(); s.lit = r.bytes(r.u32()); s.coded = r.bytes(r.u32());
        if (s.index >= n || s.lit.size() > msl || s.coded.size() % 4) { fprintf(stderr, "work file: bad stream %u\n", s.index); exit(2); }
        osz[s.index] = (uint32_t)s.lit.size(); csz[s.index] = (uint32_t)s.coded.size();
        segs[2 * (size_t)s.index + 1].last8 = s.last8;
    }
    if (r.at != r.data.size()) { fprintf(stderr, "%zu bytes behind the last stream\n", r.data.size() - r.at); exit(2); }
    const uint64_t slot = (divans_gpu_lit_encode_bound((msl + 1u) & ~1u) + 15u) & ~(uint64_t)15;
    uint64_t total = 0; uint32_t longest = 0;
    for (uint32_t s = 0; s < n; ++s) {
        ooff[s] = total; total += osz[s]; longest = std::max(longest, osz[s]);
        coff[s] = (uint64_t)(s + 1) * slot - csz[s];
        seg_begin[s] = 2 * s;
        segs[2 * (size_t)s].len = osz[s] / 2; segs[2 * (size_t)s + 1].len = osz[s] - osz[s] / 2;
        segs[2 * (size_t)s].btype = segs[2 * (size_t)s + 1].btype = cfg.btype;
    }
    seg_begin[n] = 2 * n;
    std::vector<uint8_t> expect(total + 64, 0), blank(total + 64, 0);
    for (const Listed& s : streams) if (!s.lit.empty()) memcpy(&expect[ooff[s.index]], s.lit.data(), s.lit.size());

    g_label = name;
    fakehip::set_case(name.c_str());
    std::vector<void*> mine;
    void* d_slots = nullptr;
    HIP(hipMalloc(&d_slots, (size_t)n * slot));       // lazily committed: only the pages of the listed streams are touched
    mine.push_back(d_slots);
    for (const Listed& s : streams) if (!s.coded.empty()) HIP(hipMemcpy((uint8_t*)d_slots + coff[s.index], s.coded.data(), s.coded.size(), hipMemcpyHostToDevice));
    divans_gpu_codec* codec = nullptr;
    OK(divans_gpu_codec_create(&codec, &cfg, 0, nullptr, msl));
    if (set_types) OK(divans_gpu_codec_set_block_types(codec, set_types));
    Batch b;
    b.n = n; b.longest = longest; b.expect = &expect; b.ooff = &ooff; b.osz = &osz; b.expect_status = 0;
    b.d_coded = (const uint8_t*)d_slots; b.d_coff = dev(coff, mine); b.d_csz = dev(csz, mine);
    b.d_ooff = dev(ooff, mine); b.d_osz = dev(osz, mine); b.d_seg_begin = dev(seg_begin, mine); b.d_segs = dev(segs, mine);
    printf("WORK %s: %u streams, %u with bytes, slots of %llu bytes, last coded offset %llu\n", name.c_str(), n, listed, (unsigned long long)slot, (unsigned long long)coff[n - 1]);
    for (int call = 0; call < 2; ++call) {
        b.segs = call == 1;
        g_label = name + " | " + (b.segs ? "decode_segments_batch" : "decode_batch");
        fakehip::set_case(g_label.c_str());
        b.d_out = dev(blank, mine);
        call_and_check(codec, b);
    }
    divans_gpu_codec_destroy(codec);
    for (void* p : mine) HIP(hipFree(p));
}

int main(int argc, char** argv) {
    const bool work = argc == 4 && std::string(argv[1]) == "work";
    if (argc != (work ? 4 : 3)) { fprintf(stderr, "usage: %s CASES.bin POISON | %s work WORK.bin POISON\n", argv[0], argv[0]); return 2; }
    const int poison = (int)strtol(argv[argc - 1], nullptr, 0) & 0xff;
    simt::set_poison(poison);
    fakehip::set_fresh_fill(poison);
    printf("POISON 0x%02x\n", poison);
    size_t count = 1;
    if (work) run_work(argv[2]);
    else {
        const std::vector<Case> cases = read_cases(argv[1]);
        count = cases.size();
        for (const Case& c : cases) run_case(c);
    }
    divans_gpu_trim();
    g_label = "end";
    fakehip::check_clean_end();
    simt::print_instances();
    printf("DONE %zu cases\n", count);
    return 0;
}
