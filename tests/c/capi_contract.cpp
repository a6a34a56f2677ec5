// capi_contract.cpp -- TEST HARNESS: the batch C ABI's host code (divans_amd/csrc/capi.cpp and the launchers of the .hip files, compiled
// --offload-host-only) driven on tests/c/fakehip_rt.cpp.  Every launch is checked against the launch contract there; this program
// makes the calls, scripts times and failures, and asserts what only the sequence shows (placements alive, the pool, clean ends).
//   capi_contract <scenario> <configs file> <trace file> [<sizes file>]
// scenarios: small | m6 | placement | pool | failures.  The configs file is written by tests/test_capi_launch_contract_cpu.py from
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

static divans_gpu_codec* make_codec(const Config& cf, uint32_t msl) {
    divans_gpu_codec* c = nullptr;
    const int rc = divans_gpu_codec_create(&c, &cf.cfg, 0, nullptr, msl);
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

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: capi_contract <small|m6|placement|pool|failures> <configs> <trace> [<sizes>]\n"); return 2; }
    load_configs(argv[2]);
    fakehip::open_trace(argv[3]);
    const std::string s = argv[1];
    if (s == "small") scenario_small();
    else if (s == "m6") { if (argc < 5) return 2; scenario_m6(argv[4]); }
    else if (s == "placement") scenario_placement();
    else if (s == "pool") scenario_pool();
    else if (s == "failures") scenario_failures();
    else return 2;
    printf("%s: %zu launches, contract held\n", s.c_str(), fakehip::launches().size());
    return 0;
}
