// wide_block_types_contract.cpp -- TEST HARNESS: divans_gpu_codec_set_block_types above eight types on tests/c/fakehip_rt.cpp, the
// recording HIP runtime of the launch-contract test (capi_contract.cpp is the driver of everything else).  Above eight literal block
// types a codec whose context map is not constant keeps its context tables in a second layout (divans_amd/csrc/lit_kernels.h) that
// kernel instances of their own read: overloads with one trailing template argument.  This program makes the calls at four streams on
// a plain, a mixing, a table-driven and a no-cache configuration, with 9 and with 256 types; fakehip_rt.cpp checks every launch (the
// blob's extent mix_off + 8192, the LDS per CU, the tables' extent); the program checks what the names and return codes must be.
//   wide_block_types_contract <trace file>
// A failed expectation prints EXPECTATION FAILED and exits 2; a contract violation aborts.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/divans_gpu.h"
#include "../../divans_amd/csrc/lit_kernels.h"
#include "fakehip_rt.h"

static std::string g_label;
static void label(const std::string& s) { g_label = s; fakehip::set_case(s.c_str()); }

#define EXPECT(cond, ...)                                                                                        \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            fprintf(stderr, "EXPECTATION FAILED %s:%d [%s] %s: ", __FILE__, __LINE__, g_label.c_str(), #cond);   \
            fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n");                                                 \
            exit(2);                                                                                             \
        }                                                                                                        \
    } while (0)
#define OK(call) do { const int rc_ = (call); EXPECT(rc_ == 0, "%s -> %d: %s", #call, rc_, divans_gpu_last_error()); } while (0)
#define REFUSED(call, word)                                                                                                          \
    do {                                                                                                                             \
        const size_t at_ = fakehip::launches().size();                                                                               \
        const int rc_ = (call);                                                                                                      \
        EXPECT(rc_ == DIVANS_GPU_EINVAL, "%s -> %d, expected DIVANS_GPU_EINVAL", #call, rc_);                                        \
        EXPECT(std::string(divans_gpu_last_error()).find(word) != std::string::npos, "%s: the reason is \"%s\"", #call, divans_gpu_last_error()); \
        EXPECT(fakehip::launches().size() == at_, "%s was refused after a launch", #call);                                           \
    } while (0)

static std::vector<void*> g_mine;
template <class T> static T* dev(const std::vector<T>& v) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)) != hipSuccess) { fprintf(stderr, "driver: hipMalloc failed\n"); exit(2); }
    if (!v.empty()) (void)hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    g_mine.push_back(p);
    return (T*)p;
}
static uint8_t* dev_bytes(size_t n) { return dev(std::vector<uint8_t>(std::max<size_t>(n, 16))); }

// four streams, two segments and one Literal command each, block types spread over [0, n_btypes)
struct Batch {
    uint32_t n = 4, longest = 0;
    uint64_t slot = 0;
    uint8_t *d_in, *d_back, *d_slots, *d_hist, *d_packed;
    uint64_t *d_off, *d_slot_off, *d_out_off, *d_hist_off, *d_total, *d_packed_off;
    uint32_t *d_sz, *d_coded_sz, *d_out_sz, *d_seg_begin, *d_cmd_begin, *d_lit_sz, *d_hist_sz, *d_pairs;
    divans_lit_segment* d_segs;
    divans_lit_command* d_cmds;
};
static Batch make_batch(uint32_t msl, uint32_t n_btypes) {
    Batch b;
    const std::vector<uint32_t> sizes = {msl, 1u, 0u, 117u};
    std::vector<uint64_t> off(b.n), slot_off(b.n), hist_off(b.n, 0);
    std::vector<uint32_t> coded(b.n), seg_begin(b.n + 1), cmd_begin(b.n + 1), hist_sz(b.n, 16);
    std::vector<divans_lit_segment> segs(2 * b.n + 1);
    std::vector<divans_lit_command> cmds(b.n + 1);
    std::memset(segs.data(), 0, segs.size() * sizeof(segs[0])); std::memset(cmds.data(), 0, cmds.size() * sizeof(cmds[0]));
    b.slot = divans_gpu_lit_encode_bound((msl + 1u) & ~1u);
    uint64_t total = 0;
    for (uint32_t s = 0; s < b.n; ++s) {
        off[s] = total; total += sizes[s]; b.longest = std::max(b.longest, sizes[s]);
        slot_off[s] = (uint64_t)s * b.slot;
        coded[s] = (uint32_t)std::min<uint64_t>(b.slot, ((uint64_t)sizes[s] + 3u) / 4u * 4u + 32u);
        seg_begin[s] = 2 * s; cmd_begin[s] = s;
        segs[2 * s].len = sizes[s] / 2; segs[2 * s + 1].len = sizes[s] - sizes[s] / 2;
        segs[2 * s].btype = (s * (n_btypes - 1u)) / (b.n - 1u); segs[2 * s + 1].btype = n_btypes - 1u;      // 0 .. n - 1, the last type in every stream
        cmds[s].kind = DIVANS_CMD_LITERAL; cmds[s].len = sizes[s]; cmds[s].arg = segs[2 * s].btype;
    }
    seg_begin[b.n] = 2 * b.n; cmd_begin[b.n] = b.n;
    b.d_in = dev_bytes(total + 64); b.d_back = dev_bytes(total + 64);
    b.d_slots = dev_bytes((size_t)b.n * b.slot); b.d_packed = dev_bytes((size_t)b.n * b.slot);
    b.d_off = dev(off); b.d_sz = dev(sizes); b.d_slot_off = dev(slot_off); b.d_coded_sz = dev(coded);
    b.d_out_off = dev(std::vector<uint64_t>(b.n)); b.d_out_sz = dev(std::vector<uint32_t>(b.n)); b.d_packed_off = dev(std::vector<uint64_t>(b.n));
    b.d_total = dev(std::vector<uint64_t>(1)); b.d_lit_sz = dev(sizes);
    b.d_seg_begin = dev(seg_begin); b.d_segs = dev(segs); b.d_cmd_begin = dev(cmd_begin); b.d_cmds = dev(cmds);
    b.d_hist = dev_bytes(64); b.d_hist_off = dev(hist_off); b.d_hist_sz = dev(hist_sz);
    b.d_pairs = (uint32_t*)dev_bytes((size_t)b.n * 2u * ((msl + 1u) & ~1u) * 4u);
    return b;
}

static int encode_batch(divans_gpu_codec* c, const Batch& b) { return divans_gpu_lit_encode_batch(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_slots, b.slot, b.d_out_off, b.d_out_sz); }
static int encode_segments(divans_gpu_codec* c, const Batch& b) { return divans_gpu_lit_encode_segments_batch(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_seg_begin, b.d_segs, b.d_slots, b.slot, b.d_out_off, b.d_out_sz); }
static int decode_batch(divans_gpu_codec* c, const Batch& b) { return divans_gpu_lit_decode_batch(c, b.d_slots, b.d_slot_off, b.d_coded_sz, b.n, b.d_back, b.d_off, b.d_sz, b.longest); }
static int decode_segments(divans_gpu_codec* c, const Batch& b) { return divans_gpu_lit_decode_segments_batch(c, b.d_slots, b.d_slot_off, b.d_coded_sz, b.n, b.d_seg_begin, b.d_segs, b.d_back, b.d_off, b.d_sz, b.longest); }
static int decode_commands(divans_gpu_codec* c, const Batch& b, bool hist) {
    if (hist) return divans_gpu_lit_decode_commands_history_batch(c, b.d_slots, b.d_slot_off, b.d_coded_sz, b.n, b.d_cmd_begin, b.d_cmds, b.d_lit_sz, b.longest, nullptr, nullptr, nullptr,
                                                                  b.d_back, b.d_off, b.d_sz, b.d_hist, b.d_hist_off, b.d_hist_sz);
    return divans_gpu_lit_decode_commands_batch(c, b.d_slots, b.d_slot_off, b.d_coded_sz, b.n, b.d_cmd_begin, b.d_cmds, b.d_lit_sz, b.longest, nullptr, nullptr, nullptr, b.d_back, b.d_off, b.d_sz);
}
static int encode_commands(divans_gpu_codec* c, const Batch& b, bool hist) {
    if (hist) return divans_gpu_lit_encode_commands_history_batch(c, b.d_in, b.d_off, b.d_sz, b.n, b.d_cmd_begin, b.d_cmds, b.longest, nullptr, nullptr, nullptr, b.d_slots, b.slot,
                                                                  b.d_out_off, b.d_out_sz, b.d_lit_sz, b.d_hist, b.d_hist_off, b.d_hist_sz);
    return divans_gpu_lit_encode_commands_batch(c, b.d_in, b.d_off, b.d_sz, b.n, b.d_cmd_begin, b.d_cmds, b.longest, nullptr, nullptr, nullptr, b.d_slots, b.slot, b.d_out_off, b.d_out_sz, b.d_lit_sz);
}
// what lit_commands_prepare_kernel leaves for the segment encoders (as in capi_contract.cpp)
static void prepare_effect(const fakehip::Launch& l) {
    const divans_hip::LitCommandPrepare& p = *(const divans_hip::LitCommandPrepare*)l.args.data();
    for (uint32_t s = 0; s < p.n_streams; ++s) {
        p.lit_offsets[s] = (uint64_t)s * p.lit_slot;
        p.lit_sizes[s] = std::min(p.raw_sizes[s], p.lit_stream_len);
        p.seg_begin[s] = p.cmd_begin[s] - p.cmd_first;
    }
    p.seg_begin[p.n_streams] = p.cmd_last - p.cmd_first;
}

// ---- the four configurations -------------------------------------------------------------------------------------------------------
struct Config { const char* name; divans_lit_config cfg; bool cached; int mm; };
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static Config make_config(const char* name, bool mix, bool table_driven, bool cached, bool constant = false) {
    Config c; c.name = name; c.cached = cached; c.mm = table_driven ? -1 : 4;
    divans_lit_config_context_mixing(&c.cfg);
    c.cfg.btype = 3;
    c.cfg.context_mixing = mix ? 2 : 0;
    uint32_t seed = 12345u;
    for (uint32_t t = 0; t < 256u; ++t)
        for (uint32_t i = 0; i < 64u; ++i)
            c.cfg.literal_context_map[64u * t + i] = constant ? 5u : (uint8_t)(cached ? ((2u * (t % 32u) + 1u) * i + 9u * (t / 32u)) % (table_driven ? 32u : 64u) : lcg(seed) & 0xffu);      // (two planes of rows: 32 contexts leave room for row caches)
    if (table_driven) {
        const uint8_t vals[] = {0, 2, 3, 4, 5, 6, 7, 8, 12, 15, 1};
        for (uint32_t i = 0; i < sizeof(c.cfg.mixing_mask); ++i) c.cfg.mixing_mask[i] = vals[lcg(seed) % (cached ? 10u : 11u)];     // value 1: 256 x 256 low rows, no row cache
    }
    return c;
}

static std::string decode_name(divans_gpu_codec* c, const char* entry, size_t launches_before) {
    char name[200];
    EXPECT(divans_gpu_codec_last_decode_kernel(c, name, sizeof(name)) == 0, "last_decode_kernel");
    const fakehip::Launch* hit = nullptr;
    const auto& ls = fakehip::launches();
    for (size_t i = launches_before; i < ls.size(); ++i) if (ls[i].kernel.find("lit_decode") != std::string::npos) hit = &ls[i];
    EXPECT(hit != nullptr, "%s launched no decode kernel", entry);
    EXPECT(hit->kernel == name, "%s: the library names %s, the runtime launched %s", entry, name, hit->kernel.c_str());
    fakehip::trace_note(std::string("\"entry\": \"") + entry + "\", \"kernel\": \"" + name + "\", \"grid\": " + std::to_string(hit->grid) + ", \"lds\": " + std::to_string(hit->lds));
    return name;
}
static bool ends_with(const std::string& s, const char* tail) { const size_t n = strlen(tail); return s.size() >= n && s.compare(s.size() - n, n, tail) == 0; }
// A wide instance: one template argument more than its kernel family has (5; the command kernels 4), and that argument is 1.  (The last
// argument of a fused lit_decode2_kernel instance is its cache set, which may be 1 as well: the count tells them apart.)
static bool is_wide(const std::string& k) {
    const size_t lt = k.find('<');
    if (lt == std::string::npos) return false;
    const size_t args = 1u + (size_t)std::count(k.begin() + lt, k.end(), ',');
    const size_t base = k.find("lit_decode2_cmd_") != std::string::npos ? 4u : 5u;
    EXPECT(args == base || (args == base + 1u && ends_with(k, ", 1>")), "%s has %zu template arguments", k.c_str(), args);
    return args == base + 1u;
}
static const fakehip::Launch& last_of(const char* family, size_t launches_before) {
    const auto& ls = fakehip::launches();
    const fakehip::Launch* hit = nullptr;
    for (size_t i = launches_before; i < ls.size(); ++i) if (ls[i].kernel.find(family) != std::string::npos) hit = &ls[i];
    EXPECT(hit != nullptr, "no %s launch", family);
    return *hit;
}

// every list entry point; `wide`: the launched kernels must carry the trailing argument (and must not when the layout is the fused one)
static void list_entry_points(divans_gpu_codec* c, const Config& cf, const Batch& b, bool wide, const std::string& base) {
    const std::string mmv = std::to_string(cf.mm);
    size_t at = fakehip::launches().size();
    label(base + "/encode_segments");
    OK(encode_segments(c, b));
    {
        const std::string k = last_of("lit_model_encode_kernel", at).kernel;
        EXPECT(is_wide(k) == wide && ends_with(k, wide ? ", true, 1>" : ", true>"), "encode_segments launched %s", k.c_str());
        EXPECT(k.find("lit_model_encode_kernel<" + mmv + ", ") != std::string::npos, "encode_segments launched %s", k.c_str());
        uint32_t ran = 0; OK(divans_gpu_codec_last_encode_path(c, &ran));
        EXPECT(ran == 1u, "a list on path 0 is coded by the streaming kernels, ran %u", ran);
    }
    label(base + "/decode_segments");
    at = fakehip::launches().size();
    OK(decode_segments(c, b));
    {
        const std::string k = decode_name(c, "decode_segments_batch", at);
        EXPECT(k.find("lit_decode2_kernel_") != std::string::npos && is_wide(k) == wide, "decode_segments launched %s", k.c_str());
        if (wide) EXPECT(k.find("lit_decode2_kernel_any<" + mmv + ", false, ") != std::string::npos, "decode_segments launched %s", k.c_str());
        if (wide) EXPECT(ends_with(k, ", 0, 1>") == !cf.cached, "the row caches of %s", k.c_str());
    }
    for (int hist = 0; hist < 2; ++hist) {
        label(base + (hist ? "/encode_commands_history" : "/encode_commands"));
        at = fakehip::launches().size();
        OK(encode_commands(c, b, hist != 0));
        const std::string ke = last_of("lit_model_encode_kernel", at).kernel;
        EXPECT(is_wide(ke) == wide, "encode_commands launched %s", ke.c_str());
        label(base + (hist ? "/decode_commands_history" : "/decode_commands"));
        at = fakehip::launches().size();
        OK(decode_commands(c, b, hist != 0));
        const std::string k = decode_name(c, hist ? "decode_commands_history_batch" : "decode_commands_batch", at);
        EXPECT(k.find(hist ? "lit_decode2_cmd_hist_kernel<" : "lit_decode2_cmd_kernel<") != std::string::npos && is_wide(k) == wide, "decode_commands launched %s", k.c_str());
    }
}

static void wide_codec(const Config& cf, uint32_t n_btypes) {
    const std::string base = std::string(cf.name) + "/bt" + std::to_string(n_btypes);
    label(base);
    const uint32_t msl = 300;
    divans_gpu_codec* c = nullptr;
    OK(divans_gpu_codec_create(&c, &cf.cfg, 0, nullptr, msl));
    REFUSED(divans_gpu_codec_set_block_types(c, 0), "1..256");
    REFUSED(divans_gpu_codec_set_block_types(c, 257), "1..256");
    OK(divans_gpu_codec_set_block_types(c, n_btypes));
    uint32_t slots = 99;
    OK(divans_gpu_codec_high_row_slots(c, &slots));
    EXPECT(slots == 0u, "a wide codec has no slot table, high_row_slots reports %u", slots);
    const Batch b = make_batch(msl, n_btypes);
    list_entry_points(c, cf, b, true, base);
    // a direct-mapped request comes down to the 2-way organisation (the instances that exist)
    if (cf.cached) {
        label(base + "/direct_mapped_request");
        OK(divans_gpu_codec_set_decoder(c, 2, nullptr, nullptr, 0));
        const size_t at = fakehip::launches().size();
        OK(decode_segments(c, b));
        const std::string k = decode_name(c, "decode_segments_batch", at);
        EXPECT(ends_with(k, cf.cfg.context_mixing > 1 ? ", 19, 1>" : ", 17, 1>"), "generation 2 on a wide list launched %s", k.c_str());
    }
    // what such a codec does not do
    label(base + "/refusals");
    REFUSED(divans_gpu_codec_set_encode_path(c, 2), "bucketed");
    REFUSED(encode_batch(c, b), "without segment lists");
    REFUSED(decode_batch(c, b), "without segment lists");
    REFUSED(divans_gpu_lit_model_batch(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_pairs), "divans_gpu_lit_model_batch");
    REFUSED(divans_gpu_lit_encode_packed(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_packed, (uint64_t)b.n * b.slot, b.d_packed_off, b.d_out_sz, b.d_total, 0), "without segment lists");
    REFUSED(divans_gpu_lit_stream_begin(c), "call by call");
    REFUSED(divans_gpu_lit_stream_decode_begin(c), "call by call");
    float ms = 0.f;
    REFUSED(divans_gpu_codec_row_replay(c, b.d_in, b.d_off, b.d_sz, b.n, b.longest, &ms), "divans_gpu_codec_row_replay");
    // eight types again: the fused layout, the old instances, the calls without lists
    label(base + "/back_to_8");
    OK(divans_gpu_codec_set_block_types(c, 8));
    const Batch b8 = make_batch(msl, 8);
    list_entry_points(c, cf, b8, false, base + "/back_to_8");
    OK(encode_batch(c, b8));
    OK(decode_batch(c, b8));
    uint32_t status = 0;
    OK(divans_gpu_codec_status(c, &status));
    divans_gpu_codec_destroy(c);
}

// a constant context at 256 types: no wide instance, the pass and the calls the codec has at eight types
static void constant_codec() {
    const Config cf = make_config("constant", false, false, true, true);
    label("constant/bt256");
    divans_gpu_codec* c = nullptr;
    OK(divans_gpu_codec_create(&c, &cf.cfg, 0, nullptr, 300));
    OK(divans_gpu_codec_set_block_types(c, 256));
    const Batch b = make_batch(300, 256);
    const size_t first = fakehip::launches().size();
    OK(divans_gpu_codec_set_encode_path(c, 2));
    OK(encode_segments(c, b));
    uint32_t ran = 0; OK(divans_gpu_codec_last_encode_path(c, &ran));
    EXPECT(ran == 2u, "the bucketed pass of a constant context at 256 types, ran %u", ran);
    OK(divans_gpu_codec_set_encode_path(c, 0));
    OK(encode_segments(c, b)); OK(encode_batch(c, b)); OK(decode_batch(c, b)); OK(decode_segments(c, b));
    for (int hist = 0; hist < 2; ++hist) { OK(encode_commands(c, b, hist != 0)); OK(decode_commands(c, b, hist != 0)); }
    const auto& ls = fakehip::launches();
    size_t lit = 0;
    for (size_t i = first; i < ls.size(); ++i) {
        const std::string& k = ls[i].kernel;
        if (k.find("lit_model_encode_kernel") == std::string::npos && k.find("lit_decode") == std::string::npos) continue;
        ++lit;
        EXPECT(!is_wide(k) && k.find("<4, true, ") != std::string::npos, "a constant context launched %s", k.c_str());
    }
    EXPECT(lit >= 7u, "%zu streaming launches", lit);      // (the call without lists on path 0 takes the bucketed pass)
    divans_gpu_codec_destroy(c);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: wide_block_types_contract <trace>\n"); return 2; }
    fakehip::open_trace(argv[1]);
    fakehip::set_effect("lit_commands_prepare", prepare_effect);
    const Config configs[] = {make_config("plain", false, false, true), make_config("mixing", true, false, true),
                              make_config("table_driven", true, true, true), make_config("no_cache", false, true, false)};
    for (const Config& cf : configs)
        for (uint32_t n : {9u, 256u}) wide_codec(cf, n);
    constant_codec();
    for (void* p : g_mine) (void)hipFree(p);
    g_mine.clear();
    divans_gpu_trim();
    fakehip::check_clean_end();
    printf("wide block types: %zu launches, contract held\n", fakehip::launches().size());
    return 0;
}
