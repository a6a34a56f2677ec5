// capi_contract.cpp -- TEST HARNESS: the batch C ABI's host code (divans_amd/csrc/capi.cpp and the launchers of the .hip files, compiled
// --offload-host-only) driven on tests/c/fakehip_rt.cpp.  Every launch is checked against the launch contract there; this program
// makes the calls, scripts times and failures, and asserts what only the sequence shows (placements alive, the pool, clean ends).
//   capi_contract <scenario> <configs file> <trace file> [<sizes file>]
// scenarios: small | m6 | placement | pool | failures (codecs on the null stream) | streams_small | streams_placement | streams_host
// (codecs on a non-blocking stream of the driver's).  The configs file is written by tests/test_capi_launch_contract_cpu.py from
// the table of tests/test_gpu_encode_dispatch.py: records of {char name[32]; u32 types (~0: as created); u32 path_2_before_types;
// u32 btype; u32 reserved; divans_lit_config}.  A failed expectation prints EXPECTATION FAILED and exits 2; a contract violation aborts.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/divans_gpu.h"
#include "../../divans_amd/csrc/lit_kernels.h"
#include "fakehip_rt.h"

#define EXPECT(cond, ...)                                                                                        \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            fprintf(stderr, "EXPECTATION FAILED %s:%d [%s] %s: ", __FILE__, __LINE__, g_label.c_str(), #cond);   \
            fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n");                                                 \
            exit(2);                                                                                             \
        }                                                                                                        \
    } while (0)

static std::string g_label;
static void label(const std::string& s) { g_label = s; fakehip::set_case(s.c_str()); }

struct Config { std::string name; uint32_t types, path_2_before_types, btype; divans_lit_config cfg; };
static std::vector<Config> g_configs;
static const Config& config(const std::string& name) {
    for (const Config& c : g_configs) if (c.name == name) return c;
    fprintf(stderr, "no configuration %s\n", name.c_str()); exit(2);
}
static void load_configs(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    struct { char name[32]; uint32_t types, p2, btype, reserved; } head;
    while (fread(&head, sizeof(head), 1, f) == 1) {
        Config c; c.name = head.name; c.types = head.types; c.path_2_before_types = head.p2; c.btype = head.btype;
        if (fread(&c.cfg, sizeof(c.cfg), 1, f) != 1) { fprintf(stderr, "short configs file\n"); exit(2); }
        g_configs.push_back(c);
    }
    fclose(f);
    Config s; s.name = "simple"; s.types = ~0u; s.path_2_before_types = 0; divans_lit_config_simple(&s.cfg); s.btype = s.cfg.btype; g_configs.push_back(s);
    Config m; m.name = "mixing"; m.types = ~0u; m.path_2_before_types = 0; divans_lit_config_context_mixing(&m.cfg); m.btype = m.cfg.btype; g_configs.push_back(m);
}

// the driver's own device arrays
static std::vector<void*> g_mine;
template <class T> static T* dev(const std::vector<T>& v) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)) != hipSuccess) { fprintf(stderr, "driver: hipMalloc failed\n"); exit(2); }
    if (!v.empty()) (void)hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    g_mine.push_back(p);
    return (T*)p;
}
static uint8_t* dev_bytes(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 16)) != hipSuccess) { fprintf(stderr, "driver: hipMalloc(%zu) failed\n", n); exit(2); }
    g_mine.push_back(p);
    return (uint8_t*)p;
}
static void free_mine() { for (void* p : g_mine) (void)hipFree(p); g_mine.clear(); }

// One batch with everything the entry points take.  No kernel runs, so the coded sizes are made up (a multiple of 4 inside the slot).
struct Batch {
    uint32_t n = 0, longest = 0, msl = 0;
    uint64_t slot = 0;
    std::vector<uint32_t> sizes;
    uint8_t *d_in = nullptr, *d_back = nullptr, *d_slots = nullptr, *d_packed = nullptr, *d_hist = nullptr;
    uint64_t *d_off = nullptr, *d_slot_off = nullptr, *d_out_off = nullptr, *d_hist_off = nullptr, *d_total = nullptr, *d_packed_off = nullptr;
    uint32_t *d_sz = nullptr, *d_coded_sz = nullptr, *d_out_sz = nullptr, *d_seg_begin = nullptr, *d_cmd_begin = nullptr, *d_lit_sz = nullptr, *d_hist_sz = nullptr, *d_pairs = nullptr;
    divans_lit_segment* d_segs = nullptr;
    divans_lit_command* d_cmds = nullptr;
    uint64_t total = 0;
};
static Batch make_batch(const std::vector<uint32_t>& sizes, uint32_t msl, uint32_t btype, bool pairs = true) {
    Batch b;
    b.n = (uint32_t)sizes.size(); b.sizes = sizes; b.msl = msl;
    std::vector<uint64_t> off(b.n), slot_off(b.n), hist_off(b.n, 0);
    std::vector<uint32_t> coded(b.n), seg_begin(b.n + 1), cmd_begin(b.n + 1), hist_sz(b.n, 16);
    std::vector<divans_lit_segment> segs(2 * (size_t)b.n + 1);
    std::vector<divans_lit_command> cmds((size_t)b.n + 1);
    std::memset(segs.data(), 0, segs.size() * sizeof(segs[0])); std::memset(cmds.data(), 0, cmds.size() * sizeof(cmds[0]));
    b.slot = divans_gpu_lit_encode_bound((msl + 1u) & ~1u);
    for (uint32_t s = 0; s < b.n; ++s) {
        off[s] = b.total; b.total += sizes[s]; b.longest = std::max(b.longest, sizes[s]);
        slot_off[s] = (uint64_t)s * b.slot;
        coded[s] = (uint32_t)std::min<uint64_t>(b.slot, ((uint64_t)sizes[s] + 3u) / 4u * 4u + 32u);
        seg_begin[s] = 2 * s; cmd_begin[s] = s;
        segs[2 * s].len = sizes[s] / 2; segs[2 * s + 1].len = sizes[s] - sizes[s] / 2; segs[2 * s].btype = segs[2 * s + 1].btype = btype;
        cmds[s].kind = DIVANS_CMD_LITERAL; cmds[s].len = sizes[s]; cmds[s].arg = btype;
    }
    seg_begin[b.n] = 2 * b.n; cmd_begin[b.n] = b.n;
    b.d_in = dev_bytes(b.total + 64); b.d_back = dev_bytes(b.total + 64);
    b.d_slots = dev_bytes((size_t)b.n * b.slot); b.d_packed = dev_bytes((size_t)b.n * b.slot);
    b.d_off = dev(off); b.d_sz = dev(sizes); b.d_slot_off = dev(slot_off); b.d_coded_sz = dev(coded);
    b.d_out_off = dev(std::vector<uint64_t>(b.n)); b.d_out_sz = dev(std::vector<uint32_t>(b.n)); b.d_packed_off = dev(std::vector<uint64_t>(b.n));
    b.d_total = dev(std::vector<uint64_t>(1)); b.d_lit_sz = dev(sizes);
    b.d_seg_begin = dev(seg_begin); b.d_segs = dev(segs); b.d_cmd_begin = dev(cmd_begin); b.d_cmds = dev(cmds);
    b.d_hist = dev_bytes(64); b.d_hist_off = dev(hist_off); b.d_hist_sz = dev(hist_sz);
    if (pairs) b.d_pairs = (uint32_t*)dev_bytes((size_t)b.n * 2u * ((msl + 1u) & ~1u) * 4u);
    return b;
}

// the stream every codec of the run is created on: null in scenarios 1-5, a non-blocking stream of the driver's in the streams_* ones
static hipStream_t g_stream = nullptr;
static divans_gpu_codec* make_codec(const Config& cf, uint32_t msl) {
    divans_gpu_codec* c = nullptr;
    const int rc = divans_gpu_codec_create(&c, &cf.cfg, 0, g_stream, msl);
    EXPECT(rc == 0 && c, "codec_create: %d %s", rc, divans_gpu_last_error());
    return c;
}

// the decode kernel the library says it launched is the one the runtime saw
static void note_decode(divans_gpu_codec* c, const char* entry, size_t launches_before) {
    char name[160];
    EXPECT(divans_gpu_codec_last_decode_kernel(c, name, sizeof(name)) == 0, "last_decode_kernel");
    const auto& ls = fakehip::launches();
    const fakehip::Launch* hit = nullptr;
    for (size_t i = launches_before; i < ls.size(); ++i) if (ls[i].kernel.find("lit_decode") != std::string::npos) hit = &ls[i];
    EXPECT(hit != nullptr, "%s launched no decode kernel", entry);
    EXPECT(hit->kernel == name, "%s: the library names %s, the runtime launched %s", entry, name, hit->kernel.c_str());
    fakehip::trace_note(std::string("\"entry\": \"") + entry + "\", \"kernel\": \"" + name + "\", \"grid\": " + std::to_string(hit->grid) + ", \"lds\": " + std::to_string(hit->lds) +
                        ", \"tables\": \"" + (hit->tables_kind == fakehip::KIND_CHUNK ? "chunks" : "block") + "\", \"tables_id\": " + std::to_string(hit->tables_born));
}
static void note_encode(divans_gpu_codec* c, const char* entry, uint32_t path) {
    uint32_t ran = 0;
    EXPECT(divans_gpu_codec_last_encode_path(c, &ran) == 0, "last_encode_path");
    fakehip::trace_note(std::string("\"entry\": \"") + entry + "\", \"path\": " + std::to_string(path) + ", \"ran\": " + std::to_string(ran));
}

#define OK(call) do { const int rc_ = (call); EXPECT(rc_ == 0, "%s -> %d: %s", #call, rc_, divans_gpu_last_error()); } while (0)

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

// EFFECT (tests/c/README.md): what lit_commands_prepare_kernel leaves for the segment encoders, which the host hands on as their input
static void prepare_effect(const fakehip::Launch& l) {
    const divans_hip::LitCommandPrepare& p = *(const divans_hip::LitCommandPrepare*)l.args.data();
    for (uint32_t s = 0; s < p.n_streams; ++s) {
        p.lit_offsets[s] = (uint64_t)s * p.lit_slot;
        p.lit_sizes[s] = std::min(p.raw_sizes[s], p.lit_stream_len);
        p.seg_begin[s] = p.cmd_begin[s] - p.cmd_first;
    }
    p.seg_begin[p.n_streams] = p.cmd_last - p.cmd_first;
}

static std::vector<uint32_t> ragged(uint32_t n, uint32_t longest) {
    std::vector<uint32_t> v(n);
    for (uint32_t i = 0; i < n; ++i) v[i] = i == 5 ? 0u : 1u + (i * 37u) % longest;
    v[0] = longest;
    return v;
}

static void clean_end() {
    divans_gpu_trim();
    divans_gpu_table_memory_info mi;
    OK(divans_gpu_table_memory(&mi));
    EXPECT(mi.va_reserved_bytes == fakehip::reserved_bytes(), "divans_gpu_table_memory reports %llu reserved, the runtime handed out %zu", (unsigned long long)mi.va_reserved_bytes, fakehip::reserved_bytes());
    EXPECT(mi.idle_ranges == 0, "idle ranges after trim");
    free_mine();
    fakehip::check_clean_end();
}

// ---- scenario 1: every entry point at small shapes -----------------------------------------------------------------------------
static void every_entry_point(const Config& cf, const char* shape, bool full_grid) {
    const uint32_t longest = 300;
    divans_gpu_codec* c = make_codec(cf, longest);
    if (cf.path_2_before_types) OK(divans_gpu_codec_set_encode_path(c, 2));
    if (cf.types != ~0u) OK(divans_gpu_codec_set_block_types(c, cf.types));
    divans_gpu_info info;
    OK(divans_gpu_codec_info(c, &info));
    const uint32_t n = full_grid ? info.resident_groups + 1u : 37u;
    Batch b = make_batch(ragged(n, longest), longest, cf.btype);
    const std::string base = cf.name + "/" + shape;
    label(base + "/decode");
    fakehip::trace_note("\"entry\": \"info\", \"n_streams\": " + std::to_string(n) + ", \"resident_groups\": " + std::to_string(info.resident_groups) + ", \"blocks\": " + std::to_string(info.blocks) +
                        ", \"rows_per_stream\": " + std::to_string(info.rows_per_stream));
    for (uint32_t path = 0; path < 3; ++path) {
        label(base + "/path" + std::to_string(path));
        const int rc = divans_gpu_codec_set_encode_path(c, path);
        fakehip::trace_note("\"entry\": \"set_encode_path\", \"path\": " + std::to_string(path) + ", \"accepted\": " + (rc == 0 ? "true" : "false"));
        OK(encode_batch(c, b)); note_encode(c, "encode_batch", path);
        OK(encode_segments(c, b)); note_encode(c, "encode_segments_batch", path);
        OK(divans_gpu_lit_model_batch(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_pairs)); note_encode(c, "model_batch", path);
        OK(divans_gpu_lit_encode_packed(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_packed, (uint64_t)b.n * b.slot, b.d_packed_off, b.d_out_sz, b.d_total, full_grid ? 8192u : 16u)); note_encode(c, "encode_packed", path);
        for (int hist = 0; hist < 2; ++hist) { OK(encode_commands(c, b, hist != 0)); note_encode(c, hist ? "encode_commands_history_batch" : "encode_commands_batch", path); }
    }
    label(base + "/decode");
    size_t at = fakehip::launches().size();
    OK(decode_batch(c, b)); note_decode(c, "decode_batch", at);
    at = fakehip::launches().size();
    OK(decode_segments(c, b)); note_decode(c, "decode_segments_batch", at);
    for (int hist = 0; hist < 2; ++hist) {
        at = fakehip::launches().size();
        const int rc = decode_commands(c, b, hist != 0);
        if (rc == 0) note_decode(c, hist ? "decode_commands_history_batch" : "decode_commands_batch", at);
        else EXPECT(rc == DIVANS_GPU_EINVAL && fakehip::launches().size() == at, "decode_commands: %d %s", rc, divans_gpu_last_error());      // generation 1 codecs (wrap-checked speeds)
    }
    float ms = 0.f;
    at = fakehip::launches().size();
    const int rr = divans_gpu_codec_row_replay(c, b.d_in, b.d_off, b.d_sz, b.n, b.longest, &ms);
    EXPECT(rr == 0 || rr == DIVANS_GPU_EINVAL, "row_replay: %d %s", rr, divans_gpu_last_error());
    fakehip::trace_note(std::string("\"entry\": \"row_replay\", \"ran\": ") + (rr == 0 ? "true" : "false"));
    uint32_t status = 0;
    OK(divans_gpu_codec_status(c, &status));
    divans_gpu_codec_destroy(c);
}
// caches of 256 high rows: 141 KiB of LDS a workgroup, one workgroup a CU -- the launches that need hipFuncSetAttribute
static void big_caches(const Config& cf) {
    label(cf.name + "/big_caches/decode");
    divans_gpu_codec* c = make_codec(cf, 300);
    const bool mix = cf.cfg.context_mixing > 1;      // with mixing the high rows are two tables: stride and context-map rows
    const uint32_t rows[4] = {mix ? 128u : 256u, mix ? 128u : 0u, 0, 0}, shifts[4] = {5, 5, 0, 0};
    OK(divans_gpu_codec_set_decoder(c, 2, rows, shifts, 0));
    divans_gpu_info info;
    OK(divans_gpu_codec_info(c, &info));
    Batch b = make_batch(ragged(info.resident_groups + 1u, 300), 300, cf.btype, false);
    size_t at = fakehip::launches().size();
    OK(decode_batch(c, b)); note_decode(c, "decode_batch", at);
    EXPECT(fakehip::launches().back().lds > 65536u || fakehip::launches()[at].lds > 65536u, "the case was written for more than 64 KiB of LDS");
    at = fakehip::launches().size();
    OK(decode_segments(c, b)); note_decode(c, "decode_segments_batch", at);
    for (int hist = 0; hist < 2; ++hist) { at = fakehip::launches().size(); OK(decode_commands(c, b, hist != 0)); note_decode(c, hist ? "decode_commands_history_batch" : "decode_commands_batch", at); }
    divans_gpu_codec_destroy(c);
    free_mine();
}
// a larger batch behind a smaller one that is still enqueued: every grow-only work buffer is given back and allocated anew
static void buffers_grow(const Config& cf) {
    label(cf.name + "/buffers_grow");
    divans_gpu_codec* c = make_codec(cf, 300);
    if (cf.types != ~0u) OK(divans_gpu_codec_set_block_types(c, cf.types));
    Batch few = make_batch(ragged(37, 300), 300, cf.btype), more = make_batch(ragged(101, 300), 300, cf.btype);
    for (uint32_t path = 1; path <= 2; ++path) {
        OK(divans_gpu_codec_set_encode_path(c, path));
        for (const Batch* b : {&few, &more}) {
            OK(encode_batch(c, *b)); OK(encode_segments(c, *b)); OK(encode_commands(c, *b, false));
            OK(divans_gpu_lit_encode_packed(c, b->d_in, b->d_off, b->d_sz, b->longest, b->n, b->d_packed, (uint64_t)b->n * b->slot, b->d_packed_off, b->d_out_sz, b->d_total, 0));
        }
    }
    divans_gpu_codec_destroy(c);
    free_mine();
}
static void scenario_small() {
    fakehip::set_effect("lit_commands_prepare", prepare_effect);
    buffers_grow(config("stride_1"));
    buffers_grow(config("two_model"));
    big_caches(config("simple"));
    big_caches(config("mixing"));
    for (const Config& cf : g_configs) {
        if (cf.name == "simple" || cf.name == "mixing") continue;
        every_entry_point(cf, "ragged37", false);
        every_entry_point(cf, "full_grid", true);
        free_mine();
    }
    clean_end();
}

// ---- scenario 2: the sequence of test_work_arrays_past_4g, with m6 behind the three families it runs today -------------------------
static void work_sequence(const Config& cf, const Batch& b) {
    divans_gpu_codec* c = make_codec(cf, 65536);
    if (cf.types != ~0u) OK(divans_gpu_codec_set_block_types(c, cf.types));
    OK(divans_gpu_codec_set_bucket_batch(c, b.n));
    for (uint32_t path = 1; path <= 2; ++path) {
        label(cf.name + "/work/path" + std::to_string(path));
        OK(divans_gpu_codec_set_encode_path(c, path));
        OK(encode_batch(c, b)); note_encode(c, "encode_batch", path);
        OK(encode_segments(c, b)); note_encode(c, "encode_segments_batch", path);
        OK(divans_gpu_lit_model_batch(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_pairs)); note_encode(c, "model_batch", path);
        uint32_t status = 0;
        OK(divans_gpu_codec_status(c, &status));
        size_t at = fakehip::launches().size();
        OK(decode_batch(c, b)); note_decode(c, "decode_batch", at);
        OK(divans_gpu_codec_status(c, &status));
        at = fakehip::launches().size();
        OK(decode_segments(c, b)); note_decode(c, "decode_segments_batch", at);
        OK(divans_gpu_codec_status(c, &status));
        divans_gpu_table_placement pl;
        OK(divans_gpu_codec_table_placement(c, &pl));
        divans_gpu_info info;
        OK(divans_gpu_codec_info(c, &info));
        fakehip::trace_note("\"entry\": \"placement\", \"tried\": " + std::to_string(pl.tried) + ", \"searching\": " + std::to_string(pl.searching) + ", \"table_bytes\": " + std::to_string(info.table_bytes));
    }
    divans_gpu_codec_destroy(c);
    divans_gpu_table_memory_info mi;
    OK(divans_gpu_table_memory(&mi));
    fakehip::trace_note("\"entry\": \"pool\", \"idle_ranges\": " + std::to_string(mi.idle_ranges) + ", \"idle_bytes\": " + std::to_string(mi.idle_bytes) + ", \"reserved\": " + std::to_string(mi.va_reserved_bytes));
}
static void scenario_m6(const char* sizes_path) {
    fakehip::set_capacity((size_t)288 << 30);      // an MI355X
    FILE* f = fopen(sizes_path, "rb");
    if (!f) { perror(sizes_path); exit(2); }
    std::vector<uint32_t> sizes(32840);
    EXPECT(fread(sizes.data(), 4, sizes.size(), f) == sizes.size(), "sizes file");
    fclose(f);
    Batch b = make_batch(sizes, 65536, 0);
    for (const char* name : {"simple", "mixing", "context_keyed"}) {
        Config cf = config(name);
        if (cf.name != "context_keyed") cf.types = ~0u;
        // the segment lists name the configuration's own block type
        std::vector<divans_lit_segment> segs(2 * (size_t)b.n + 1);
        (void)hipMemcpy(segs.data(), b.d_segs, segs.size() * sizeof(segs[0]), hipMemcpyDeviceToHost);
        for (auto& s : segs) s.btype = cf.cfg.btype;
        (void)hipMemcpy(b.d_segs, segs.data(), segs.size() * sizeof(segs[0]), hipMemcpyHostToDevice);
        work_sequence(cf, b);
    }
    Config m6 = config("stride_3");
    m6.name = "m6";
    std::vector<divans_lit_segment> segs(2 * (size_t)b.n + 1);
    (void)hipMemcpy(segs.data(), b.d_segs, segs.size() * sizeof(segs[0]), hipMemcpyDeviceToHost);
    for (auto& s : segs) s.btype = m6.cfg.btype;
    (void)hipMemcpy(b.d_segs, segs.data(), segs.size() * sizeof(segs[0]), hipMemcpyHostToDevice);
    work_sequence(m6, b);
    clean_end();
}

// ---- scenario 3: the placement search ----------------------------------------------------------------------------------------------
// tables alive: blocks of exactly `bytes`, and reserved ranges with chunks mapped that hold at least `bytes`
static uint32_t table_copies(size_t bytes) {
    uint32_t copies = 0;
    std::vector<uint64_t> ranges;
    for (const fakehip::LedgerEntry& e : fakehip::ledger()) {
        if (!e.alive) continue;
        if (e.kind == fakehip::KIND_BLOCK && e.bytes == bytes) ++copies;
        if (e.kind == fakehip::KIND_CHUNK && std::find(ranges.begin(), ranges.end(), e.born) == ranges.end()) { ranges.push_back(e.born); ++copies; }
    }
    return copies;
}
// The two-copy rule AT the moment of every allocation, not after a call: the most device memory alive since reset_peak() is what was
// there before the codec (`base`), two copies of the tables (a mapped copy is rounded up to whole 32 MiB chunks) and `slack` for the
// codec's other buffers.  A candidate allocated before the loser is freed shows as a third copy here even if it is gone on return.
static void expect_two_copies_at_most(size_t base, size_t table_bytes, size_t slack, const std::string& what) {
    const size_t peak = fakehip::peak_live_bytes() - base, allowed = 2u * (table_bytes + ((size_t)32 << 20)) + slack;
    EXPECT(slack < table_bytes && peak <= allowed, "%s: %zu bytes of device memory were alive at one point, two copies of the tables and the other buffers come to %zu at most", what.c_str(), peak, allowed);
}
static const fakehip::Launch& last_decode_launch() {
    const auto& ls = fakehip::launches();
    for (size_t i = ls.size(); i-- > 0;) if (ls[i].kernel.find("lit_decode2_kernel") != std::string::npos) return ls[i];
    fprintf(stderr, "no decode launch\n"); exit(2);
}
static void scenario_placement() {
    Config cf = config("stride_3");      // 6144 rows a stream: 3.75 GiB of tables on the full grid, mapped chunks by default
    const uint32_t n = 20481;
    Batch b = make_batch(ragged(n, 64), 64, cf.cfg.btype, false), other = make_batch(ragged(n - 1, 64), 64, cf.cfg.btype, false);
    {   // call by call: 4 candidates, scripted times, a call of another shape in between
        label("placement/search");
        const size_t base = fakehip::live_bytes();
        fakehip::reset_peak();
        divans_gpu_codec* c = make_codec(cf, 64);
        OK(divans_gpu_codec_set_block_types(c, 8));
        OK(divans_gpu_codec_search_tables(c, 4));
        fakehip::script_times("lit_decode2_kernel", {5.f, 3.f, 9.f /* other shape */, 4.f, 2.f, 7.f, 7.f});
        divans_gpu_info info;
        OK(divans_gpu_codec_info(c, &info));
        const size_t tb = info.table_bytes;
        std::vector<int> kinds; std::vector<uint64_t> ids;
        uint64_t syncs = fakehip::stream_syncs();
        for (int call = 0; call < 6; ++call) {
            if (call == 2) {      // another shape: decoded on the placement in use, not compared; the next step must wait for the stream
                const uint64_t id = last_decode_launch().tables_born;
                OK(decode_batch(c, other));
                EXPECT(last_decode_launch().tables_born == id, "a call of another shape moved the tables");
                EXPECT(fakehip::stream_syncs() == syncs, "a call of another shape synchronised the stream");
            }
            OK(decode_batch(c, b));
            const uint64_t now = fakehip::stream_syncs();
            EXPECT(now - syncs == (call == 2 ? 1u : 0u), "call %d: %llu stream synchronisations (one is needed after a call of another shape, none otherwise)", call, (unsigned long long)(now - syncs));
            syncs = now;
            EXPECT(table_copies(tb) <= 2u, "call %d: %u copies of the tables are alive", call, table_copies(tb));
            expect_two_copies_at_most(base, tb, (size_t)64 << 20, "search, call " + std::to_string(call));
            kinds.push_back(last_decode_launch().tables_kind); ids.push_back(last_decode_launch().tables_born);
            fakehip::trace_note("\"entry\": \"search_call\", \"call\": " + std::to_string(call) + ", \"tables\": \"" + (kinds.back() == fakehip::KIND_CHUNK ? "chunks" : "block") + "\", \"copies\": " + std::to_string(table_copies(tb)));
        }
        divans_gpu_table_placement pl;
        OK(divans_gpu_codec_table_placement(c, &pl));
        EXPECT(pl.tried == 4 && pl.searching == 0 && pl.best_ms == 2.f && pl.worst_ms == 5.f && pl.first_ms == 5.f, "tried %u searching %u best %g worst %g first %g", pl.tried, pl.searching, pl.best_ms, pl.worst_ms, pl.first_ms);
        EXPECT(kinds[0] == fakehip::KIND_CHUNK && kinds[1] == fakehip::KIND_BLOCK && kinds[2] == fakehip::KIND_CHUNK && kinds[3] == fakehip::KIND_BLOCK, "block and chunk candidates alternate");
        EXPECT(ids[4] == ids[3] && ids[5] == ids[3] && pl.kept_chunks == 0u, "the fastest candidate (the fourth, 2 ms) stays");
        EXPECT(table_copies(tb) == 1u, "one copy once the search is over");
        divans_gpu_codec_destroy(c);
    }
    {   // the eager form
        label("placement/eager");
        const size_t base = fakehip::live_bytes();
        fakehip::reset_peak();
        divans_gpu_codec* c = make_codec(cf, 64);
        OK(divans_gpu_codec_set_block_types(c, 8));
        OK(divans_gpu_codec_tune_tables(c, 3));
        fakehip::script_times("lit_decode2_kernel", {5.f, 3.f, 4.f});
        const size_t at = fakehip::launches().size();
        OK(decode_batch(c, b));
        divans_gpu_table_placement pl;
        OK(divans_gpu_codec_table_placement(c, &pl));
        EXPECT(pl.tried == 3 && pl.best_ms == 3.f && pl.worst_ms == 5.f && pl.kept_chunks == 0u, "eager: tried %u best %g worst %g kept_chunks %u", pl.tried, pl.best_ms, pl.worst_ms, pl.kept_chunks);
        EXPECT(fakehip::launches().size() - at == 3u, "one decode per candidate");
        divans_gpu_info info; OK(divans_gpu_codec_info(c, &info));
        EXPECT(table_copies(info.table_bytes) == 1u, "eager: the losers' memory is back");
        expect_two_copies_at_most(base, info.table_bytes, (size_t)64 << 20, "eager: every loser is freed before the next candidate is allocated");
        divans_gpu_codec_destroy(c);
    }
    {   // a candidate's allocation fails: the search ends on the best so far
        label("placement/allocation_fails");
        const size_t base = fakehip::live_bytes();
        fakehip::reset_peak();
        divans_gpu_codec* c = make_codec(cf, 64);
        OK(divans_gpu_codec_set_block_types(c, 8));
        OK(divans_gpu_codec_search_tables(c, 4));
        fakehip::script_times("lit_decode2_kernel", {5.f, 3.f});
        OK(decode_batch(c, b));
        OK(decode_batch(c, b));
        fakehip::fail_call("hipMemAddressReserve", 1, hipErrorOutOfMemory); fakehip::fail_call("hipMemAddressReserve", 2, hipErrorOutOfMemory);
        fakehip::fail_call("hipMalloc", 1, hipErrorOutOfMemory); fakehip::fail_call("hipMalloc", 2, hipErrorOutOfMemory);
        OK(decode_batch(c, b));
        fakehip::clear_failures();
        divans_gpu_table_placement pl;
        OK(divans_gpu_codec_table_placement(c, &pl));
        EXPECT(pl.tried == 2 && pl.searching == 0 && pl.best_ms == 3.f && pl.kept_chunks == 0u, "tried %u searching %u best %g kept_chunks %u", pl.tried, pl.searching, pl.best_ms, pl.kept_chunks);
        { divans_gpu_info info; OK(divans_gpu_codec_info(c, &info)); expect_two_copies_at_most(base, info.table_bytes, (size_t)64 << 20, "a candidate that cannot be allocated"); }
        divans_gpu_codec_destroy(c);
    }
    clean_end();
}

// ---- scenario 4: the pool ------------------------------------------------------------------------------------------------------------
static void scenario_pool() {
    Config cf = config("stride_3");
    Batch b = make_batch(ragged(37, 64), 64, cf.cfg.btype, false);
    auto big = [&](uint32_t blocks) {      // tables of blocks * 16 * 6144 * 32 bytes
        divans_gpu_codec* c = make_codec(cf, 64);
        OK(divans_gpu_codec_set_block_types(c, 8));
        OK(divans_gpu_codec_tune_tables(c, 1));
        if (blocks) OK(divans_gpu_codec_set_geometry(c, blocks, 0xffffffffu));
        return c;
    };
    auto tables_of = [&](divans_gpu_codec* c) { OK(decode_batch(c, b)); return last_decode_launch(); };
    divans_gpu_table_memory_info mi;
    label("pool/small_tables_are_one_block");
    { divans_gpu_codec* c = big(600); EXPECT(tables_of(c).tables_kind == fakehip::KIND_BLOCK, "tables under 2 GiB are one block"); divans_gpu_codec_destroy(c); }
    label("pool/keeps_two");
    divans_gpu_codec* c1 = big(1280); const uint64_t r1 = tables_of(c1).tables_born;
    divans_gpu_codec* c2 = big(1100); const uint64_t r2 = tables_of(c2).tables_born;
    divans_gpu_codec* c3 = big(700);  const uint64_t r3 = tables_of(c3).tables_born;
    EXPECT(tables_of(c1).tables_kind == fakehip::KIND_CHUNK && r1 != r2 && r2 != r3, "big tables are mapped ranges of their own");
    divans_gpu_codec_destroy(c1); divans_gpu_codec_destroy(c2); divans_gpu_codec_destroy(c3);
    OK(divans_gpu_table_memory(&mi));
    EXPECT(mi.idle_ranges == 2 && mi.va_reserved_bytes == fakehip::reserved_bytes(), "two idle ranges are kept (%u), reserved %llu / %zu", mi.idle_ranges, (unsigned long long)mi.va_reserved_bytes, fakehip::reserved_bytes());
    for (const fakehip::LedgerEntry& e : fakehip::ledger()) EXPECT(!(e.kind == fakehip::KIND_CHUNK && e.born == r1), "the oldest idle range is the one evicted");
    label("pool/bound");
    {   // idle: r2 (3328 MiB) and r3 (2112 MiB).  690 blocks need 2070 MiB: r3 fits, r2 lies beyond need * 1.5 + 64 MiB
        divans_gpu_codec* c = big(690);
        EXPECT(tables_of(c).tables_born == r3, "the idle range that fits is reused");
        size_t reserved = fakehip::reserved_bytes();
        divans_gpu_codec* f = big(690);           // r2 is still idle and still too large: a new range
        const fakehip::Launch lf = tables_of(f);
        EXPECT(lf.tables_kind == fakehip::KIND_CHUNK && lf.tables_born != r2 && fakehip::reserved_bytes() > reserved, "a range beyond need * 1.5 + 64 MiB is not picked");
        reserved = fakehip::reserved_bytes();
        divans_gpu_codec* d = big(1000);          // 3000 MiB: r2 is within the bound
        EXPECT(tables_of(d).tables_born == r2 && fakehip::reserved_bytes() == reserved, "a range within need * 1.5 + 64 MiB is reused");
        divans_gpu_codec_destroy(d); divans_gpu_codec_destroy(c); divans_gpu_codec_destroy(f);      // idle: r3 (2112 MiB), then f's (2080 MiB); r2 evicted
        OK(divans_gpu_table_memory(&mi));
        EXPECT(mi.idle_ranges == 2, "two idle ranges");
        label("pool/smallest_fit");
        divans_gpu_codec* g = big(683);           // 2049 MiB: both fit, the younger one is the smaller
        EXPECT(tables_of(g).tables_born == lf.tables_born, "the pick is the smallest idle range that fits");
        divans_gpu_codec_destroy(g);
    }
    label("pool/fresh_is_never_from_the_pool");
    {   // a search's candidates are `fresh`: with two fitting ranges idle, the first tables come from the pool, the chunk candidate does not
        Batch half = make_batch(ragged(683 * 16, 64), 64, cf.cfg.btype, false);
        divans_gpu_codec* c = big(683);
        OK(divans_gpu_codec_search_tables(c, 3));
        const size_t reserved = fakehip::reserved_bytes();
        OK(decode_batch(c, half)); const fakehip::Launch first = last_decode_launch();
        EXPECT(first.tables_kind == fakehip::KIND_CHUNK && fakehip::reserved_bytes() == reserved, "the first tables come from the pool");
        OK(decode_batch(c, half)); EXPECT(last_decode_launch().tables_kind == fakehip::KIND_BLOCK, "the second placement is one block");
        OK(decode_batch(c, half));
        EXPECT(last_decode_launch().tables_kind == fakehip::KIND_CHUNK && fakehip::reserved_bytes() > reserved, "a fresh chunk candidate is never served from the pool");
        OK(decode_batch(c, half));
        divans_gpu_codec_destroy(c);
    }
    label("pool/va_cap");
    {
        OK(divans_gpu_table_memory(&mi));
        divans_gpu_trim();
        divans_gpu_set_table_va_cap(mi.va_reserved_bytes);      // spent: new tables are plain blocks
        divans_gpu_codec* c = big(1280);
        const size_t reserved = fakehip::reserved_bytes();
        EXPECT(tables_of(c).tables_kind == fakehip::KIND_BLOCK && fakehip::reserved_bytes() == reserved, "past the address-space cap tables are plain blocks");
        divans_gpu_codec_destroy(c);
        divans_gpu_set_table_va_cap((uint64_t)256 << 30);
    }
    label("pool/device_alloc_drops_idle_ranges");
    {
        divans_gpu_codec* c = big(1280); (void)tables_of(c); divans_gpu_codec_destroy(c);
        OK(divans_gpu_table_memory(&mi));
        EXPECT(mi.idle_ranges == 1, "one idle range");
        Batch w = make_batch(ragged(4000, 65536), 65536, 0, false);           // start/freq spill: 4000 * 512 KiB = 2 GiB
        fakehip::set_capacity(fakehip::live_bytes() + ((size_t)1 << 30));      // room for 1 GiB more; the idle range holds 3.75 GiB
        divans_gpu_codec* d = make_codec(config("simple"), 65536);
        OK(divans_gpu_codec_set_encode_path(d, 1));
        OK(encode_batch(d, w));
        OK(divans_gpu_table_memory(&mi));
        EXPECT(mi.idle_ranges == 0, "device_alloc gave the idle ranges back before it gave up");
        divans_gpu_codec_destroy(d);
        fakehip::set_capacity((size_t)288 << 30);
    }
    clean_end();
}

// ---- scenario 5: the failure sweep -----------------------------------------------------------------------------------------------
struct Op { const char* name; int (*run)(divans_gpu_codec*, const Batch&); uint32_t path; };
static int op_decode(divans_gpu_codec* c, const Batch& b) { return decode_batch(c, b); }
static int op_encode(divans_gpu_codec* c, const Batch& b) { return encode_batch(c, b); }
static int op_dec_cmd(divans_gpu_codec* c, const Batch& b) { return decode_commands(c, b, false); }
static int op_enc_cmd(divans_gpu_codec* c, const Batch& b) { return encode_commands(c, b, true); }

// one run: create, three calls (the placement search is two calls deep), two good calls, destroy; fail_index 0 = the good run.
// Returns the injectable calls made up to the end of the third call -- the part of the run a failure is injected into: until the
// failure fires a run is the good run, so every index up to that count fires.  *fired counts the injected failures that fired,
// *reported those of them a call returned an error for.
static uint64_t sweep_run(const Config& cf, bool mapped, const Op& op, const Batch& b, uint64_t fail_index, uint64_t* fired, uint64_t* reported) {
    const size_t live0 = fakehip::live_bytes();
    const uint64_t calls0 = fakehip::injectable_calls();
    uint64_t calls_in_window = 0;
    fakehip::reset_peak();
    fakehip::clear_failures();
    if (fail_index) fakehip::fail_at(fail_index, fail_index % 3 == 0 ? hipErrorOutOfMemory : hipErrorLaunchFailure);
    divans_gpu_codec* c = nullptr;
    int rc = divans_gpu_codec_create(&c, &cf.cfg, 0, nullptr, 64);
    bool failed = rc != 0;
    if (rc == 0) {
        int worst = 0;
        auto step = [&](int r) { if (r && !worst) worst = r; };
        step(divans_gpu_codec_set_block_types(c, cf.types == ~0u ? 1u : cf.types));
        if (mapped) step(divans_gpu_codec_search_tables(c, 3));
        else step(divans_gpu_codec_set_geometry(c, 64, 0xffffffffu));      // 192 MiB of tables: one block
        step(divans_gpu_codec_set_encode_path(c, op.path));
        for (int i = 0; i < 3; ++i) step(op.run(c, b));
        calls_in_window = fakehip::injectable_calls() - calls0;
        failed = worst != 0;
        if (failed) EXPECT(worst == DIVANS_GPU_EHIP || worst == DIVANS_GPU_ENOMEM, "%s: code %d is not one of the documented kinds (%s)", op.name, worst, divans_gpu_last_error());
        if (fail_index && *fakehip::injected_function() && !failed) {
            // absorbed on purpose: an allocation the library has a fallback for (a table candidate, chunks -> one block, a retry after the pool is dropped)
            const std::string fn = fakehip::injected_function();
            EXPECT(fn == "hipMalloc" || fn == "hipMemCreate" || fn == "hipMemMap" || fn == "hipMemAddressReserve", "%s: a failed %s went unreported", op.name, fn.c_str());
        }
        if (fired && *fakehip::injected_function()) ++*fired;
        fakehip::clear_failures();
        if (failed) (void)hipGetLastError();
        uint32_t status = 0;
        OK(divans_gpu_codec_status(c, &status));
        divans_gpu_info info;
        OK(divans_gpu_codec_info(c, &info));
        for (int i = 0; i < 2; ++i) {
            OK(op.run(c, b));
            if (mapped) EXPECT(table_copies(info.table_bytes) <= 2u, "%s after a failure at call %llu: %u copies of the tables are alive", op.name, (unsigned long long)fail_index, table_copies(info.table_bytes));
        }
        // (the encoders' work arrays for 20 481 streams come to 2 GiB; the tables are 4.5)
        if (mapped) expect_two_copies_at_most(live0, info.table_bytes, (size_t)3 << 30, std::string(op.name) + " with a failure at call " + std::to_string(fail_index));
        divans_gpu_codec_destroy(c);
    } else {
        EXPECT(rc == DIVANS_GPU_EHIP || rc == DIVANS_GPU_ENOMEM, "codec_create: %d", rc);
        if (fired && *fakehip::injected_function()) ++*fired;
        fakehip::clear_failures();
    }
    if (reported) *reported += failed ? 1u : 0u;
    divans_gpu_trim();
    EXPECT(fakehip::live_bytes() == live0, "%s, %s tables, failure at injectable call %llu (%s): %zu bytes of device memory leaked", op.name, mapped ? "mapped" : "small",
           (unsigned long long)fail_index, fakehip::injected_function(), fakehip::live_bytes() - live0);
    return calls_in_window;
}
constexpr uint64_t kSweepEveryCallBelow = 2000;      // "thousands of calls": below that every call is failed
static void scenario_failures() {
    fakehip::set_effect("lit_commands_prepare", prepare_effect);
    divans_gpu_set_table_va_cap((uint64_t)1 << 62);      // hundreds of codecs with mapped tables: none of them may end on the plain-block policy
    const Op ops[] = {{"decode_batch", op_decode, 0}, {"encode_batch path 1", op_encode, 1}, {"encode_batch path 2", op_encode, 2},
                      {"decode_commands_batch", op_dec_cmd, 0}, {"encode_commands_history_batch", op_enc_cmd, 1}};
    const Config cf = config("stride_3");
    Batch small = make_batch(ragged(37, 64), 64, cf.cfg.btype, false), full = make_batch(ragged(20481, 64), 64, cf.cfg.btype, false);
    for (int mapped = 0; mapped < 2; ++mapped) {
        for (const Op& op : ops) {
            const Batch& b = mapped ? full : small;
            label(std::string("failures/") + (mapped ? "mapped/" : "small/") + op.name);
            const uint64_t good = sweep_run(cf, mapped != 0, op, b, 0, nullptr, nullptr);
            uint64_t fired = 0, reported = 0, runs = 0;
            // every call the good run makes up to the end of its third call; only where those are thousands, the first and last 50 and every 7th between
            for (uint64_t k = 1; k <= good; ++k) {
                if (good >= kSweepEveryCallBelow && k > 50 && k + 50 <= good && k % 7) continue;
                (void)sweep_run(cf, mapped != 0, op, b, k, &fired, &reported); ++runs;
            }
            EXPECT(fired == runs, "%llu of %llu injected failures fired", (unsigned long long)fired, (unsigned long long)runs);
            fakehip::trace_note("\"entry\": \"sweep\", \"op\": \"" + std::string(op.name) + "\", \"mapped\": " + (mapped ? "true" : "false") + ", \"calls\": " + std::to_string(good) +
                                ", \"runs\": " + std::to_string(runs) + ", \"fired\": " + std::to_string(fired) + ", \"reported\": " + std::to_string(reported) +
                                ", \"every_call_below\": " + std::to_string(kSweepEveryCallBelow));
        }
    }
    {   // the case of its own: the launch behind placement_step's swap fails, and the same shape is called again
        label("failures/placement_swap_then_launch_fails");
        for (const char* fn : {"hipLaunchKernel", "hipEventRecord"}) {
            const size_t live0 = fakehip::live_bytes();
            fakehip::reset_peak();
            divans_gpu_codec* c = make_codec(cf, 64);
            OK(divans_gpu_codec_set_block_types(c, 8));
            OK(divans_gpu_codec_search_tables(c, 4));
            fakehip::script_times("lit_decode2_kernel", {5.f, 6.f, 7.f, 8.f});
            OK(decode_batch(c, full));                                   // placement 0, measured
            const uint64_t best = last_decode_launch().tables_born;
            fakehip::fail_call(fn, 1, hipErrorLaunchFailure);
            const int rc = decode_batch(c, full);                        // candidate 1 swapped in, then the call fails
            EXPECT(rc == DIVANS_GPU_EHIP, "the failed call returns %d", rc);
            (void)hipGetLastError();
            divans_gpu_info info; OK(divans_gpu_codec_info(c, &info));
            for (int i = 0; i < 6; ++i) {
                OK(decode_batch(c, full));
                EXPECT(table_copies(info.table_bytes) <= 2u, "%s failed after the swap: %u copies of the tables alive at the call %d after it", fn, table_copies(info.table_bytes), i);
                expect_two_copies_at_most(live0, info.table_bytes, (size_t)64 << 20, std::string(fn) + " failed after the swap, call " + std::to_string(i) + " after it");
            }
            divans_gpu_table_placement pl;
            OK(divans_gpu_codec_table_placement(c, &pl));
            EXPECT(pl.searching == 0 && pl.best_ms == 5.f, "searching %u best %g: the measured best (5 ms) is what the search ends on", pl.searching, pl.best_ms);
            EXPECT(last_decode_launch().tables_born == best, "the placement that measured best is the one kept");
            divans_gpu_codec_destroy(c);
            divans_gpu_trim();
            EXPECT(fakehip::live_bytes() == live0, "%s failed after the swap: %zu bytes leaked", fn, fakehip::live_bytes() - live0);
        }
    }
    clean_end();
}

// ---- scenarios 6-8: the same ABI on a caller's NON-BLOCKING stream (tests/c/README.md, "The stream model") --------------------------
// On such a stream nothing the library enqueues is complete, as far as the host can see, until the library (or the driver) waits:
// the destination of every device-to-host copy keeps its old bytes until then, and a synchronous copy, a free or a map that meets
// an entry still in flight is an `order` / `lifetime` violation.  The effects below stand for the kernels whose results the host
// reads back; what they write depends on the driver's call counter, so a value left over from an earlier call is a wrong value.
static uint32_t g_call = 0;                                   // bumped by the driver in front of every call whose results it checks
static uint32_t g_bad_stream_at = ~0u, g_bad_model_at = ~0u;  // the call whose decode / rANS launch raises its status bit
static uint32_t coded_size(uint32_t s, uint32_t call) { return 4u * (1u + (s + call) % 5u); }
static uint8_t coded_byte(uint32_t call) { return (uint8_t)(0x41u + call % 23u); }
static uint8_t decoded_byte(uint32_t s, uint32_t call) { return (uint8_t)((0x61u + call % 19u) ^ (s << 5)); }
static uint32_t consumed_words(uint32_t call) { return 1u + call % 7u; }
static void rans_effect(const fakehip::Launch& l) {
    const divans_hip::RansBatch& r = *(const divans_hip::RansBatch*)l.args.data();
    for (uint32_t s = 0; s < r.n_streams; ++s) {
        const uint32_t size = (uint32_t)std::min<uint64_t>(coded_size(s, g_call), r.out_slot);
        r.out_sizes[s] = size; r.out_offsets[s] = (uint64_t)s * r.out_slot + r.out_slot - size;
        std::memset(r.out + r.out_offsets[s], coded_byte(g_call), size);
        if (r.chunk_bytes) r.chunk_bytes[(size_t)s * r.max_chunks] = size;
    }
    if (g_bad_model_at == g_call) *r.status |= DIVANS_GPU_STATUS_BAD_MODEL;      // where the real pass meets an invalid (start, freq)
}
static void decode_effect(const fakehip::Launch& l) {
    const divans_hip::LitBatch& b = *(const divans_hip::LitBatch*)l.args.data();
    for (uint32_t s = 0; s < b.n_streams; ++s) {
        const uint64_t off = b.out_offsets ? b.out_offsets[s] : (uint64_t)s * b.stream_len;
        std::memset(b.out + off, decoded_byte(s, g_call), b.out_sizes ? b.out_sizes[s] : b.stream_len);
        if (b.consumed) b.consumed[s] = consumed_words(g_call);
    }
    if (g_bad_stream_at == g_call) { *b.status |= DIVANS_GPU_STATUS_BAD_STREAM; if (b.stream_bad && b.n_streams > 3) b.stream_bad[3] = 1; }
}
// the pack pass as the kernels do it (lit_kernels.hip, scan_sizes_kernel / pack_copy_kernel): what encode_packed, the host wrappers
// and the caller read back is then the sum and the bytes of THIS call's sizes
static void scan_effect(const fakehip::Launch& l) {
    const fakehip::ScanArgs& a = *(const fakehip::ScanArgs*)l.args.data();
    uint64_t run = a.accumulate ? *a.total : 0;
    for (uint32_t i = 0; i < a.n; ++i) { a.offsets[i] = run; run += (a.sizes[i] + 3u) & ~3u; }
    *a.total = run;
}
static void pack_effect(const fakehip::Launch& l) {
    const fakehip::PackArgs& a = *(const fakehip::PackArgs*)l.args.data();
    for (uint32_t s = 0; s < a.n; ++s) {
        const uint64_t bytes = ((uint64_t)a.sizes[s] + 3u) & ~3ull;
        if (a.dst_off[s] + bytes > a.cap) { if (a.status) *a.status |= DIVANS_GPU_STATUS_OUTPUT_FULL; continue; }
        std::memcpy(a.packed + a.dst_off[s], a.slots + a.src_off[s], a.sizes[s]);
    }
}
static void stream_effects() {
    fakehip::set_effect("lit_commands_prepare", prepare_effect);
    fakehip::set_effect("rans_", rans_effect);
    fakehip::set_effect("lit_decode", decode_effect);
    fakehip::set_effect("scan_sizes_kernel", scan_effect);
    fakehip::set_effect("pack_copy_kernel", pack_effect);
}

static void non_blocking_stream() {
    if (hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking) != hipSuccess) { fprintf(stderr, "driver: hipStreamCreateWithFlags failed\n"); exit(2); }
    EXPECT(fakehip::stream_kind(g_stream) == fakehip::STREAM_NON_BLOCKING, "the driver's stream is not a non-blocking one");
}
static void drop_stream() {
    EXPECT(fakehip::pending_entries(g_stream) == 0, "%zu entries of the caller's stream are still in flight at the end", fakehip::pending_entries(g_stream));
    (void)hipStreamDestroy(g_stream); g_stream = nullptr;
}

// every value a call under test reads back is this call's, not the previous call's and not the buffer's first contents
struct HostOut {
    std::vector<uint8_t> packed; std::vector<uint64_t> off; std::vector<uint32_t> sz, chunks; size_t total = 0x5a5a5a5a;
    explicit HostOut(uint32_t n, size_t cap) : packed(cap, 0xEE), off(n, 0xEEEEEEEEEEEEEEEEull), sz(n, 0xEEEEEEEEu), chunks((size_t)n * 2u, 0xEEEEEEEEu) {}
};
// what an encode wrapper returns for `n` streams coded in slices of `S` (the effects number a slice's streams from 0)
static void expect_encoded(const char* what, uint32_t call, uint32_t n, uint32_t S, const uint8_t* packed, const uint64_t* off, const uint32_t* sz, size_t total, const uint32_t* chunks) {
    uint64_t run = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t want = coded_size(s % S, call);
        EXPECT(sz[s] == want, "%s, call %u: size of stream %u is %u, this call's launch wrote %u (the previous call's: %u)", what, call, s, sz[s], want, coded_size(s % S, call - 1));
        EXPECT(off[s] == run, "%s, call %u: offset of stream %u is %llu, not %llu", what, call, s, (unsigned long long)off[s], (unsigned long long)run);
        for (uint32_t k = 0; k < want; ++k) EXPECT(packed[run + k] == coded_byte(call), "%s, call %u: byte %u of stream %u is 0x%02x, this call's launch wrote 0x%02x", what, call, k, s, packed[run + k], coded_byte(call));
        if (chunks) EXPECT(chunks[2u * s] == want && chunks[2u * s + 1u] == 0u, "%s, call %u: chunk sizes of stream %u are %u, %u", what, call, s, chunks[2u * s], chunks[2u * s + 1u]);
        run += want;      // sizes are multiples of 4
    }
    EXPECT(total == run, "%s, call %u: total %zu, this call's launches come to %llu", what, call, total, (unsigned long long)run);
}
static void expect_decoded(const char* what, uint32_t call, uint32_t n, uint32_t S, uint32_t len, const uint8_t* out) {
    for (uint32_t s = 0; s < n; ++s) for (uint32_t k = 0; k < len; k += len - 1u)
        EXPECT(out[(size_t)s * len + k] == decoded_byte(s % S, call), "%s, call %u: byte %u of stream %u is 0x%02x, this call's launch wrote 0x%02x", what, call, k, s, out[(size_t)s * len + k], decoded_byte(s % S, call));
}
static void host_entry_points(const Config& cf) {
    const uint32_t n = 37, len = 300;
    const std::string base = cf.name + "/host";
    divans_gpu_codec* c = make_codec(cf, 40000);
    std::vector<uint8_t> in((size_t)n * len, 0x20);
    const size_t cap = (size_t)n * divans_gpu_lit_encode_bound(len);
    std::vector<uint64_t> last_off; std::vector<uint32_t> last_sz; std::vector<uint8_t> last_packed;
    for (int round = 0; round < 2; ++round) {      // every buffer and the codec are used twice: a stale read returns the other round's well-formed values
        label(base + "/encode_host");
        { HostOut o(n, cap); ++g_call;
          OK(divans_gpu_lit_encode_host(c, in.data(), len, n, o.packed.data(), cap, o.off.data(), o.sz.data(), &o.total));
          expect_encoded("encode_host", g_call, n, n, o.packed.data(), o.off.data(), o.sz.data(), o.total, nullptr); }
        label(base + "/encode_host_chunks");
        { HostOut o(n, cap); ++g_call;
          OK(divans_gpu_lit_encode_host_chunks(c, in.data(), len, n, o.packed.data(), cap, o.off.data(), o.sz.data(), &o.total, o.chunks.data(), 2));
          expect_encoded("encode_host_chunks", g_call, n, n, o.packed.data(), o.off.data(), o.sz.data(), o.total, o.chunks.data());
          last_off = o.off; last_sz = o.sz; last_packed = o.packed; }
        label(base + "/encode_host/bad_model");
        { HostOut o(n, cap); ++g_call; g_bad_model_at = g_call;
          const int rc = divans_gpu_lit_encode_host(c, in.data(), len, n, o.packed.data(), cap, o.off.data(), o.sz.data(), &o.total);
          EXPECT(rc == DIVANS_GPU_EINVAL, "the call whose model launch raised BAD_MODEL returns %d", rc);
          ++g_call;
          OK(divans_gpu_lit_encode_host(c, in.data(), len, n, o.packed.data(), cap, o.off.data(), o.sz.data(), &o.total));      // the word was this call's own again
          expect_encoded("encode_host after a refused call", g_call, n, n, o.packed.data(), o.off.data(), o.sz.data(), o.total, nullptr); }
        label(base + "/decode_host");
        { std::vector<uint8_t> out((size_t)n * len, 0xEE); ++g_call;
          OK(divans_gpu_lit_decode_host(c, last_packed.data(), last_off.data(), last_sz.data(), n, out.data(), len));
          expect_decoded("decode_host", g_call, n, n, len, out.data());
          ++g_call; g_bad_stream_at = g_call;
          const int rc = divans_gpu_lit_decode_host(c, last_packed.data(), last_off.data(), last_sz.data(), n, out.data(), len);
          EXPECT(rc == DIVANS_GPU_ECORRUPT, "the call whose decode launch raised BAD_STREAM returns %d", rc);
          ++g_call;
          OK(divans_gpu_lit_decode_host(c, last_packed.data(), last_off.data(), last_sz.data(), n, out.data(), len));
          expect_decoded("decode_host after a refused call", g_call, n, n, len, out.data()); }
        for (uint32_t S : {37u, 13u, 6u}) for (int pinned = 0; pinned < 2; ++pinned) {      // 1, 3 and 7 slices, into page-locked and into pageable memory
            label(base + "/pipelined/" + std::to_string((n + S - 1u) / S) + (pinned ? "_slices_pinned" : "_slices_pageable"));
            HostOut o(n, cap);
            uint8_t* h_in = pinned ? (uint8_t*)divans_gpu_host_alloc(in.size()) : in.data();
            uint8_t* h_packed = pinned ? (uint8_t*)divans_gpu_host_alloc(cap) : o.packed.data();
            uint8_t* h_out = pinned ? (uint8_t*)divans_gpu_host_alloc(in.size()) : nullptr;
            std::vector<uint8_t> out_pageable(in.size(), 0xEE);
            if (!h_out) h_out = out_pageable.data();
            EXPECT(h_in && h_packed && h_out, "divans_gpu_host_alloc");
            if (pinned) { std::memcpy(h_in, in.data(), in.size()); std::memset(h_packed, 0xEE, cap); std::memset(h_out, 0xEE, in.size()); }
            ++g_call;
            OK(divans_gpu_lit_encode_host_pipelined(c, h_in, len, n, h_packed, cap, o.off.data(), o.sz.data(), &o.total, S));
            expect_encoded("encode_host_pipelined", g_call, n, S, h_packed, o.off.data(), o.sz.data(), o.total, nullptr);
            ++g_call;
            OK(divans_gpu_lit_decode_host_pipelined(c, h_packed, o.off.data(), o.sz.data(), n, h_out, len, S));
            expect_decoded("decode_host_pipelined", g_call, n, S, len, h_out);
            ++g_call; g_bad_stream_at = g_call;
            const int rc = divans_gpu_lit_decode_host_pipelined(c, h_packed, o.off.data(), o.sz.data(), n, h_out, len, S);
            EXPECT(rc == DIVANS_GPU_ECORRUPT, "the pipelined call whose decode launch raised BAD_STREAM returns %d", rc);
            if (pinned) { divans_gpu_host_free(h_in); divans_gpu_host_free(h_packed); divans_gpu_host_free(h_out); }
        }
    }
    // one stream piece by piece: 20 000 + 20 000 bytes complete one 65 536-symbol chunk, _finish codes the open one
    for (int round = 0; round < 2; ++round) {
        label(base + "/stream_encode");
        std::vector<uint8_t> piece(20000, 0x33), out(divans_gpu_lit_encode_bound(65536), 0xEE);
        uint32_t sizes[4] = {0xEEEEEEEEu, 0xEEEEEEEEu, 0, 0}, chunks = 99; size_t out_len = 0x5a5a;
        OK(divans_gpu_lit_stream_begin(c));
        ++g_call;
        OK(divans_gpu_lit_stream_encode(c, piece.data(), 20000, 0, out.data(), out.size(), sizes, 4, &chunks, &out_len));
        EXPECT(chunks == 0 && out_len == 0, "the first piece completes no chunk (%u, %zu)", chunks, out_len);
        ++g_call;
        OK(divans_gpu_lit_stream_encode(c, piece.data(), 20000, 0x0807060504030201ull, out.data(), out.size(), sizes, 4, &chunks, &out_len));
        EXPECT(chunks == 1 && sizes[0] == coded_size(0, g_call) && out_len == sizes[0] && out[0] == coded_byte(g_call) && out[out_len - 1] == coded_byte(g_call),
               "stream_encode, call %u: %u chunks, size %u (this call's launch wrote %u), %zu bytes, first 0x%02x", g_call, chunks, sizes[0], coded_size(0, g_call), out_len, out[0]);
        ++g_call; out_len = 0x5a5a;
        OK(divans_gpu_lit_stream_finish(c, out.data(), out.size(), &out_len));
        EXPECT(out_len == coded_size(0, g_call) && out[0] == coded_byte(g_call), "stream_finish, call %u: %zu bytes, first 0x%02x", g_call, out_len, out[0]);
        label(base + "/stream_decode");
        std::vector<uint8_t> coded(4096, 0x11), back(32768, 0xEE);
        OK(divans_gpu_lit_stream_decode_begin(c));
        for (int k = 0; k < 2; ++k) {
            size_t consumed = 0x5a5a; ++g_call;
            OK(divans_gpu_lit_stream_decode(c, coded.data(), coded.size(), k ? 1000u : 32768u, 0, back.data(), &consumed));
            EXPECT(consumed == 4u * consumed_words(g_call) && back[0] == decoded_byte(0, g_call) && back[k ? 999 : 32767] == decoded_byte(0, g_call),
                   "stream_decode, call %u: consumed %zu (this call's launch wrote %u words), first byte 0x%02x", g_call, consumed, consumed_words(g_call), back[0]);
        }
        ++g_call; g_bad_stream_at = g_call;
        size_t consumed = 0;
        const int rc = divans_gpu_lit_stream_decode(c, coded.data(), coded.size(), 1000u, 0, back.data(), &consumed);
        EXPECT(rc == DIVANS_GPU_ECORRUPT, "the stream_decode call whose launch raised BAD_STREAM returns %d", rc);
        // the device-pointer calls are open again once no stream is: begin + finish with nothing pending
        OK(divans_gpu_lit_stream_begin(c)); out_len = 1; OK(divans_gpu_lit_stream_finish(c, out.data(), out.size(), &out_len)); EXPECT(out_len == 0, "an empty stream finishes with %zu bytes", out_len);
    }
    {   // the primitives' test entry points copy in, launch, copy out and wait on the codec's stream as well
        label(base + "/selftests");
        uint64_t mismatches = 1; OK(divans_gpu_selftest_division(c, &mismatches));
        const uint32_t ops[8] = {6, 0, 0, 0, 6, 0, 0, 0}; int32_t rec[32];
        OK(divans_gpu_selftest_cdf_ops(c, ops, 2, rec)); OK(divans_gpu_selftest_cdf_ops_on(c, 1, ops, 2, rec));
        const uint32_t pairs[4] = {1u << 16, 1u << 16, 1u << 16, 1u << 16}; uint8_t coded[256]; size_t coded_len = 0x5a5a;
        ++g_call;
        OK(divans_gpu_selftest_rans_pairs(c, pairs, 4, coded, sizeof(coded), &coded_len));
        EXPECT(coded_len == coded_size(0, g_call) && coded[0] == coded_byte(g_call), "selftest_rans_pairs, call %u: %zu bytes, first 0x%02x", g_call, coded_len, coded[0]);
    }
    divans_gpu_codec_destroy(c);
}

// the status calls and pack_streams on the caller's stream: each reports its own launch
static void status_calls(const Config& cf) {
    label(cf.name + "/status");
    divans_gpu_codec* c = make_codec(cf, 300);
    Batch b = make_batch(ragged(37, 300), 300, cf.btype);
    uint8_t* d_flags = dev_bytes(64);
    uint32_t* h_word = (uint32_t*)divans_gpu_host_alloc(sizeof(uint32_t));
    EXPECT(h_word != nullptr, "divans_gpu_host_alloc");
    OK(divans_gpu_codec_set_stream_flags(c, d_flags));
    for (int round = 0; round < 2; ++round) {
        uint32_t status = 0xEEEEEEEEu;
        ++g_call; OK(decode_batch(c, b));
        OK(divans_gpu_codec_status(c, &status)); EXPECT(status == 0, "status after a clean decode is %u", status);
        ++g_call; g_bad_stream_at = g_call; OK(decode_batch(c, b));
        *h_word = 0xEEEEEEEEu;
        OK(divans_gpu_codec_status_async(c, h_word));
        EXPECT(*h_word == 0xEEEEEEEEu, "status_async wrote the word (%u) before anything waited: the copy is not stream-ordered", *h_word);
        EXPECT(hipStreamSynchronize(g_stream) == hipSuccess, "sync");
        EXPECT(*h_word == DIVANS_GPU_STATUS_BAD_STREAM, "status_async behind a failing decode reports %u", *h_word);
        uint8_t flags[37];
        (void)hipMemcpy(flags, d_flags, 37, hipMemcpyDeviceToHost);
        for (uint32_t s = 0; s < 37; ++s) EXPECT(flags[s] == (s == 3 ? 1 : 0), "flag of stream %u is %u", s, flags[s]);
        (void)hipMemset(d_flags, 0, 64);
        // clear_status queued behind the failing call clears its bit; a later call's bit is kept
        OK(divans_gpu_codec_clear_status(c));
        *h_word = 0xEEEEEEEEu; OK(divans_gpu_codec_status_async(c, h_word));
        ++g_call; g_bad_model_at = g_call; OK(encode_batch(c, b));
        OK(divans_gpu_codec_status(c, &status));
        EXPECT(*h_word == 0, "status_async behind clear_status reports %u", *h_word);
        EXPECT(status == DIVANS_GPU_STATUS_BAD_MODEL, "status reports %u: the bit of the call behind clear_status alone is %u", status, DIVANS_GPU_STATUS_BAD_MODEL);
        OK(divans_gpu_codec_status(c, &status)); EXPECT(status == 0, "status read twice reports %u the second time", status);
        // pack_streams on this call's sizes: total and offsets are the prefix sums of what the launch in front wrote
        ++g_call; OK(encode_batch(c, b));
        OK(divans_gpu_pack_streams(c, b.d_slots, b.d_out_off, b.d_out_sz, b.n, b.d_packed, b.d_packed_off, b.d_total));
        EXPECT(hipStreamSynchronize(g_stream) == hipSuccess, "sync");
        uint64_t total = 0, want = 0; std::vector<uint64_t> poff(b.n);
        (void)hipMemcpy(&total, b.d_total, 8, hipMemcpyDeviceToHost); (void)hipMemcpy(poff.data(), b.d_packed_off, 8u * b.n, hipMemcpyDeviceToHost);
        for (uint32_t s = 0; s < b.n; ++s) { EXPECT(poff[s] == want, "pack_streams: offset %u", s); want += coded_size(s, g_call); }
        EXPECT(total == want, "pack_streams: total %llu, this call's sizes come to %llu", (unsigned long long)total, (unsigned long long)want);
    }
    divans_gpu_codec_destroy(c);
    divans_gpu_host_free(h_word);
    free_mine();
}

// the setters with work in flight: each is called behind a launch nothing has waited for, and the same call is made again
static void setters_in_flight(const Config& cf, uint32_t types_a, uint32_t types_b) {
    label(cf.name + "/setters_in_flight");
    divans_gpu_codec* c = make_codec(cf, 300);
    OK(divans_gpu_codec_set_block_types(c, types_a));
    Batch b = make_batch(ragged(37, 300), 300, cf.btype);
    auto work = [&]() { ++g_call; OK(encode_segments(c, b)); ++g_call; OK(decode_segments(c, b)); ++g_call; OK(encode_batch(c, b)); ++g_call; OK(decode_batch(c, b)); };
    auto tried = [&](int rc, const char* what) { EXPECT(rc == 0 || rc == DIVANS_GPU_EINVAL, "%s: %d %s", what, rc, divans_gpu_last_error()); };
    const uint32_t rows[4] = {32, 0, 0, 0}, shifts[4] = {5, 5, 0, 0};
    work(); OK(divans_gpu_codec_set_block_types(c, types_b));
    work(); OK(divans_gpu_codec_set_block_types(c, types_a));
    work(); tried(divans_gpu_codec_set_geometry(c, 64, 0xffffffffu), "set_geometry");
    work(); tried(divans_gpu_codec_set_decoder(c, 3, rows, shifts, 0), "set_decoder");
    work(); tried(divans_gpu_codec_set_split_cache(c, 32, 0), "set_split_cache");
    for (uint32_t order : {2u, 1u, 0u}) { work(); OK(divans_gpu_codec_set_byte_order(c, order)); }
    work(); tried(divans_gpu_codec_set_high_row_pinning(c, 2), "set_high_row_pinning");
    work(); tried(divans_gpu_codec_set_encode_path(c, 2), "set_encode_path");
    work(); tried(divans_gpu_codec_set_bucket_batch(c, 16), "set_bucket_batch");
    work(); tried(divans_gpu_codec_set_rans_split(c, 1), "set_rans_split");
    work(); tried(divans_gpu_codec_tune_tables(c, 1), "tune_tables");
    work();
    uint32_t mode = 0, ready = 0, slots = 0, distance = 0; uint8_t rank[256]; float ms = 0.f;
    OK(divans_gpu_codec_byte_order(c, &mode, &ready, rank));
    OK(divans_gpu_codec_high_row_slots(c, &slots)); OK(divans_gpu_codec_bucket_stride(c, &distance));
    ++g_call; OK(encode_commands(c, b, false)); OK(divans_gpu_codec_last_prepare_ms(c, &ms));
    uint32_t* d_chunks = (uint32_t*)dev_bytes((size_t)b.n * 8u);
    ++g_call; OK(divans_gpu_lit_encode_batch_chunks(c, b.d_in, b.d_off, b.d_sz, b.longest, b.n, b.d_slots, b.slot, b.d_out_off, b.d_out_sz, d_chunks, 2));
    uint32_t status = 0; OK(divans_gpu_codec_status(c, &status));
    divans_gpu_codec_destroy(c);
    free_mine();
}

static void scenario_streams_small() {
    non_blocking_stream();
    stream_effects();
    scenario_small();      // scenario 1's call table, every codec on the caller's stream
    for (const char* name : {"simple", "mixing"}) { status_calls(config(name)); setters_in_flight(config(name), 8, 2); }
    setters_in_flight(config("context_keyed"), 8, 2);
    clean_end();
    drop_stream();
}
static void scenario_streams_placement() {
    non_blocking_stream();
    scenario_placement();
    drop_stream();
}
static void scenario_streams_host() {
    non_blocking_stream();
    stream_effects();
    host_entry_points(config("simple"));
    host_entry_points(config("mixing"));
    clean_end();
    drop_stream();
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: capi_contract <small|m6|placement|pool|failures|streams_small|streams_placement|streams_host> <configs> <trace> [<sizes>]\n"); return 2; }
    load_configs(argv[2]);
    fakehip::open_trace(argv[3]);
    const std::string s = argv[1];
    if (s == "small") scenario_small();
    else if (s == "m6") { if (argc < 5) return 2; scenario_m6(argv[4]); }
    else if (s == "placement") scenario_placement();
    else if (s == "pool") scenario_pool();
    else if (s == "failures") scenario_failures();
    else if (s == "streams_small") scenario_streams_small();
    else if (s == "streams_placement") scenario_streams_placement();
    else if (s == "streams_host") scenario_streams_host();
    else return 2;
    printf("%s: %zu launches, contract held\n", s.c_str(), fakehip::launches().size());
    return 0;
}
