/*
 * cdf_ops.c -- ORACLE (test infrastructure): interpreter of the CDF-operation scripts the device selftest kernels run
 * (include/divans_gpu.h: divans_gpu_selftest_cdf_ops_on).  It holds no arithmetic of its own: every op is one or more calls
 * of the orc_cdf_* / orc_weights_* functions of cdf.c and of the state step of ans.c, on two CDF rows and one Weights
 * object, and writes one 16 x i32 record.  The mixed steps follow the order of literal.c's nibble (literal.rs:230-239):
 * average with the Weights' rate, code under the mixed row, frequencies of the symbol under both models, Weights::update.
 */
#include "divans_oracle.h"
#include <string.h>

typedef struct { orc_cdf16 row[2]; orc_weights w; } ops_state;

static void ops_reset(ops_state *s) {
    orc_cdf_default(&s->row[0]);
    orc_cdf_default(&s->row[1]);
    orc_weights_init(&s->w);
}

static void put_row(int32_t *rec, const orc_cdf16 *c) {
    for (int i = 0; i < 16; ++i) rec[i] = c->cdf[i];
}
static void put_weights(int32_t *rec, const orc_weights *w) {
    rec[0] = w->model_weights[0]; rec[1] = w->model_weights[1]; rec[2] = (uint16_t)w->normalized_weight;
}
static void put_sf(int32_t *rec, const orc_sym_start_freq *sf) {
    rec[0] = (uint16_t)sf->start; rec[1] = (uint16_t)sf->freq; rec[2] = sf->sym;
}

int orc_cdf_ops_run(const uint32_t *ops, uint32_t n, int32_t *out) {
    ops_state s;
    ops_reset(&s);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t kind = ops[4 * k], a = ops[4 * k + 1], b = ops[4 * k + 2], c = ops[4 * k + 3];
        int32_t *rec = out + (size_t)16 * k;
        memset(rec, 0, 16 * sizeof(int32_t));
        switch (kind) {
        case 0: case 1: case 7: {                          /* blend of row 0 (0, 7) / row 1 (1) */
            orc_cdf16 *r = &s.row[kind == 1];
            const orc_speed sp = {(int16_t)b, (int16_t)c};
            orc_cdf_blend(r, (uint8_t)(a & 15u), sp);
            put_row(rec, r);
            break;
        }
        case 2: {                                          /* row0.average(row1, a) */
            orc_cdf16 m;
            orc_cdf_average(&s.row[0], &s.row[1], (int32_t)a, &m);
            put_row(rec, &m);
            break;
        }
        case 3: case 4: {                                  /* sym_to_start_and_freq / cdf_offset_to_sym_start_and_freq on row 0 */
            orc_sym_start_freq sf;
            if (kind == 3) orc_cdf_sym_to_start_and_freq(&s.row[0], (uint8_t)(a & 15u), &sf);
            else orc_cdf_offset_to_sym_start_and_freq(&s.row[0], (orc_prob)(a & 0x7fffu), &sf);
            put_sf(rec, &sf);
            break;
        }
        case 5: {                                          /* Weights::update([a, b], c) */
            const orc_prob probs[2] = {(orc_prob)a, (orc_prob)b};
            orc_weights_update(&s.w, probs, (orc_prob)c);
            put_weights(rec, &s.w);
            break;
        }
        case 6: ops_reset(&s); put_row(rec, &s.row[0]); break;
        case 8:                                            /* load: entry b of row a, or field b of the Weights (a == 2) */
            if (a < 2u) { s.row[a].cdf[b & 15u] = (orc_prob)c; put_row(rec, &s.row[a]); }
            else {
                if (b < 2u) s.w.model_weights[b] = (int32_t)c;
                else s.w.normalized_weight = (int16_t)c;
                put_weights(rec, &s.w);
            }
            break;
        case 9: {                                          /* one decoded nibble from the state a | b << 32; c != 0: under the mixed row */
            const uint64_t state = (uint64_t)a | ((uint64_t)b << 32);
            orc_cdf16 m = s.row[0];
            if (c) orc_cdf_average(&s.row[0], &s.row[1], (int32_t)(uint16_t)s.w.normalized_weight, &m);
            orc_sym_start_freq sf;
            orc_cdf_offset_to_sym_start_and_freq(&m, (orc_prob)(state & 0x7fffu), &sf);
            const uint64_t x = orc_ans_advance_state(state, sf.start, sf.freq);
            put_sf(rec, &sf);
            rec[3] = (int32_t)(uint32_t)x; rec[4] = (int32_t)(uint32_t)(x >> 32);
            if (c) {
                orc_sym_start_freq f0, f1;
                orc_cdf_sym_to_start_and_freq(&s.row[0], sf.sym, &f0);
                orc_cdf_sym_to_start_and_freq(&s.row[1], sf.sym, &f1);
                rec[5] = (uint16_t)f0.freq; rec[6] = (uint16_t)f1.freq; rec[7] = (uint16_t)sf.freq;
            }
            break;
        }
        case 10: {                                         /* one mixed encoded nibble: symbol a */
            orc_cdf16 m;
            orc_cdf_average(&s.row[0], &s.row[1], (int32_t)(uint16_t)s.w.normalized_weight, &m);
            orc_sym_start_freq sf, f0, f1;
            orc_cdf_sym_to_start_and_freq(&m, (uint8_t)(a & 15u), &sf);
            orc_cdf_sym_to_start_and_freq(&s.row[0], (uint8_t)(a & 15u), &f0);
            orc_cdf_sym_to_start_and_freq(&s.row[1], (uint8_t)(a & 15u), &f1);
            const orc_prob probs[2] = {f0.freq, f1.freq};
            orc_weights_update(&s.w, probs, sf.freq);
            put_sf(rec, &sf);
            rec[3] = (uint16_t)f0.freq; rec[4] = (uint16_t)f1.freq;
            put_weights(rec + 5, &s.w);
            break;
        }
        default: return -1;
        }
    }
    return 0;
}
