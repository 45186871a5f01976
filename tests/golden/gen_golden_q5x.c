/*
 * gen_golden_q5x.c — generates the Q4_1 / Q5_0 / Q5_1 weight fixtures in tests/golden/
 * ({q41,q50,q51}_*.bin and one manifest per type) from the REFERENCE CPU path, compiled out of tree against the
 * reference's ggml.c with -march=x86-64-v3, so that ggml_vec_dot_q4_1_q8_1, ggml_vec_dot_q5_0_q8_0,
 * ggml_vec_dot_q5_1_q8_1 and quantize_row_q8_0 / quantize_row_q8_1 run their AVX2 branches
 * (ggml.c:2680-2713, 2894-2916, 3144-3169, 1192-1275, 1402-1463):
 *
 *   gcc -O2 -std=c11 -w -I$REF -march=x86-64-v3 -o gen_golden_q5x \
 *       tests/golden/gen_golden_q5x.c $REF/ggml.c -lm -lpthread
 *   ./gen_golden_q5x tests/golden
 *
 * Only this source and its output are committed.  The functions are reached through
 * ggml_internal_get_quantize_fn(type).  Inputs come from a splitmix64 + Box-Muller generator of its own.  The
 * manifests have the format tests/golden_io.py reads (variants "q41", "q50", "q51").
 *
 * Block layouts (ggml.c:877-915), B bytes per 32 weights: Q4_1 d m qs[16] (20) | Q5_0 d qh[4] qs[16] (22) |
 * Q5_1 d m qh[4] qs[16] (24); activations: block_q8_0 (34) for Q5_0, block_q8_1 = f32 d, f32 s, qs[32] (40) for
 * the other two.  XB below is the activation block's size.
 *
 * Per type and K in {64, 2304, 4160} (M = 24 weight rows, N = 3 activation rows; N = 1 is row 0):
 *   w<K>_f32      the first 4 of the N(0, 0.02) weight rows         f32 [4, K]
 *   w<K>_q        quantize_row_q of all M rows                     u8  [M, B K / 32]
 *   w<K>_dequant  dequantize_row_q of the first 4 rows             f32 [4, K]
 *   x<K>_f32      N(0, 1) activations                              f32 [N, K]
 *   x<K>_q        quantize_row_q_dot of them                       u8  [N, XB K / 32]
 *   y<K>_vec_dot  vec_dot_q, AVX2                                  f32 [N, M]
 * and crafted weight rows for K = 64 (two blocks per row, written byte by byte; a type without qh / m ignores
 * that field):
 *   craft_q       u8 [R, 2 B]     craft_dequant  f32 [R, 64]
 *   craft_x_f32   f32 [NC, 64]    craft_x_q      u8 [NC, 2 XB]    craft_y  f32 [NC, R]
 *   rows: 0 qh = 0 with all-0x00 nibble bytes | qh = 0xFFFFFFFF with all-0xFF bytes
 *         1 qh = 0xAAAAAAAA with 0xF0 bytes | qh = 0xAAAAAAAA with random bytes
 *         2 qh = 0x0000FFFF | qh = 0xFFFF0000, the same random bytes (bit e is element e)
 *         3 d = m = 0 | d = m = -0                       4 d, m = fp16 bits 0x0001, 0x83FF | 0x83FF, 0x0001
 *         5 d < 0 < m, qh all ones, bytes 0x00 | m < 0 < d, qh = 0, bytes 0xFF        6 random
 *   x:    0 N(0, 1); 1 alternating +-amax (every q = +-127); 2 all +amax (sum q = 4064); 3 all zero
 */
#include "ggml.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char *g_out, *g_var;
static FILE *g_manifest;
static int g_first;

static void dump(const char *name, const void *p, size_t n, const char *dtype, const char *shape) {
    char path[1024];
    snprintf(path, sizeof path, "%s/%s_%s.bin", g_out, g_var, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path); exit(1); }
    fclose(f);
    fprintf(g_manifest, "%s    \"%s_%s\": {\"file\": \"%s_%s.bin\", \"bytes\": %zu, \"dtype\": \"%s\", \"shape\": %s}",
            g_first ? "" : ",\n", g_var, name, g_var, name, n, dtype, shape);
    g_first = 0;
}

static uint64_t splitmix64(uint64_t *s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void fill_gaussian(float *dst, size_t n, uint64_t seed, float mean, float stdv) {
    uint64_t s = seed;
    for (size_t i = 0; i < n; i += 2) {
        const double u1 = ((double)(splitmix64(&s) >> 11) + 1.0) / 9007199254740992.0;   /* (0, 1] */
        const double u2 = (double)(splitmix64(&s) >> 11) / 9007199254740992.0;           /* [0, 1) */
        const double r = sqrt(-2.0 * log(u1));
        dst[i] = mean + stdv * (float)(r * cos(6.283185307179586 * u2));
        if (i + 1 < n) dst[i + 1] = mean + stdv * (float)(r * sin(6.283185307179586 * u2));
    }
}

static int g_has_qh, g_has_min, g_B;

static void put_block(uint8_t *blk, uint16_t dbits, uint16_t mbits, uint32_t qh, const uint8_t *qs) {
    memcpy(blk, &dbits, 2);
    blk += 2;
    if (g_has_min) { memcpy(blk, &mbits, 2); blk += 2; }
    if (g_has_qh) { memcpy(blk, &qh, 4); blk += 4; }
    memcpy(blk, qs, 16);
}

static void rand_bytes(uint8_t *qs, uint64_t *s) {
    for (int j = 0; j < 16; j++) qs[j] = (uint8_t)(splitmix64(s) & 0xFF);
}

static int one_type(enum ggml_type type, const char *var, int has_qh, int has_min, uint64_t salt) {
    g_var = var;
    g_has_qh = has_qh;
    g_has_min = has_min;
    g_first = 1;
    const int B = g_B = 18 + 2 * has_min + 4 * has_qh, XB = has_min ? 40 : 34;
    const quantize_fns_t fn = ggml_internal_get_quantize_fn(type);
    char mpath[1024];
    snprintf(mpath, sizeof mpath, "%s/%s_manifest.json", g_out, var);
    g_manifest = fopen(mpath, "w");
    if (!g_manifest) { perror(mpath); return 1; }
    fprintf(g_manifest, "{\n");
    char name[64], shape[128];

    const int Ks[3] = {64, 2304, 4160};
    for (int ki = 0; ki < 3; ki++) {
        const int K = Ks[ki], M = 24, N = 3, nb = K / 32, DR = 4;
        float *wf = malloc((size_t)M * K * 4), *x = malloc((size_t)N * K * 4), *wd = malloc((size_t)DR * K * 4);
        uint8_t *wq = calloc((size_t)M * nb, B), *xq = calloc((size_t)N * nb, XB);
        float y[3 * 24];
        fill_gaussian(wf, (size_t)M * K, 0x515EED00ull + salt + K, 0.0f, 0.02f);
        fill_gaussian(x, (size_t)N * K, 0x515EED10ull + salt + K, 0.0f, 1.0f);
        for (int m = 0; m < M; m++) fn.quantize_row_q(wf + (size_t)m * K, wq + (size_t)m * nb * B, K);
        for (int n = 0; n < N; n++) fn.quantize_row_q_dot(x + (size_t)n * K, xq + (size_t)n * nb * XB, K);
        for (int m = 0; m < DR; m++) fn.dequantize_row_q(wq + (size_t)m * nb * B, wd + (size_t)m * K, K);
        for (int n = 0; n < N; n++)
            for (int m = 0; m < M; m++)
                fn.vec_dot_q(K, &y[n * M + m], wq + (size_t)m * nb * B, xq + (size_t)n * nb * XB);
        snprintf(name, sizeof name, "w%d_f32", K);
        snprintf(shape, sizeof shape, "[%d, %d]", DR, K);
        dump(name, wf, (size_t)DR * K * 4, "f32", shape);
        snprintf(name, sizeof name, "w%d_q", K);
        snprintf(shape, sizeof shape, "[%d, %d]", M, nb * B);
        dump(name, wq, (size_t)M * nb * B, "u8", shape);
        snprintf(name, sizeof name, "w%d_dequant", K);
        snprintf(shape, sizeof shape, "[%d, %d]", DR, K);
        dump(name, wd, (size_t)DR * K * 4, "f32", shape);
        snprintf(name, sizeof name, "x%d_f32", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, K);
        dump(name, x, (size_t)N * K * 4, "f32", shape);
        snprintf(name, sizeof name, "x%d_q", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, nb * XB);
        dump(name, xq, (size_t)N * nb * XB, "u8", shape);
        snprintf(name, sizeof name, "y%d_vec_dot", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, M);
        dump(name, y, (size_t)N * M * 4, "f32", shape);
        free(wf); free(x); free(wd); free(wq); free(xq);
    }

    /* crafted weight rows, K = 64 */
    enum { R = 7, NC = 4 };
    static uint8_t cw[R][48], cxq[NC][80];
    static float cx[NC][64], cd[R][64], cy[NC][R];
    memset(cw, 0, sizeof cw);
    memset(cxq, 0, sizeof cxq);
    uint8_t qs[16], *row[R];
    uint64_t s = 0x515EEDC0ull + salt;
    for (int r = 0; r < R; r++) row[r] = (uint8_t *)cw + (size_t)r * 2 * B;      /* rows packed at 2 B bytes */
    const uint16_t d_a = ggml_fp32_to_fp16(0.0123f), d_b = ggml_fp32_to_fp16(-0.75f);
    const uint16_t m_a = ggml_fp32_to_fp16(-0.31f), m_b = ggml_fp32_to_fp16(1.75f);
    memset(qs, 0x00, 16);
    put_block(row[0], d_a, m_a, 0u, qs);
    memset(qs, 0xFF, 16);
    put_block(row[0] + B, d_b, m_b, 0xFFFFFFFFu, qs);
    memset(qs, 0xF0, 16);
    put_block(row[1], d_a, m_b, 0xAAAAAAAAu, qs);
    rand_bytes(qs, &s);
    put_block(row[1] + B, d_b, m_a, 0xAAAAAAAAu, qs);
    rand_bytes(qs, &s);
    put_block(row[2], d_a, m_a, 0x0000FFFFu, qs);
    put_block(row[2] + B, d_a, m_a, 0xFFFF0000u, qs);
    rand_bytes(qs, &s);
    put_block(row[3], 0x0000, 0x0000, (uint32_t)splitmix64(&s), qs);
    put_block(row[3] + B, 0x8000, 0x8000, (uint32_t)splitmix64(&s), qs);
    rand_bytes(qs, &s);
    put_block(row[4], 0x0001, 0x83FF, (uint32_t)splitmix64(&s), qs);
    put_block(row[4] + B, 0x83FF, 0x0001, (uint32_t)splitmix64(&s), qs);
    memset(qs, 0x00, 16);
    put_block(row[5], d_b, m_b, 0xFFFFFFFFu, qs);
    memset(qs, 0xFF, 16);
    put_block(row[5] + B, d_a, m_a, 0u, qs);
    for (int b = 0; b < 2; b++) {
        rand_bytes(qs, &s);
        put_block(row[6] + B * b, ggml_fp32_to_fp16(b ? 0.004f : 3.5f), ggml_fp32_to_fp16(b ? -0.06f : 40.0f),
                  (uint32_t)splitmix64(&s), qs);
    }
    fill_gaussian(cx[0], 64, 0x515EEDC1ull + salt, 0.0f, 1.0f);
    for (int j = 0; j < 64; j++) { cx[1][j] = (j & 1) ? -3.0f : 3.0f; cx[2][j] = 0.37f; cx[3][j] = 0.0f; }
    uint8_t *xrow[NC];
    for (int n = 0; n < NC; n++) xrow[n] = (uint8_t *)cxq + (size_t)n * 2 * XB;
    for (int n = 0; n < NC; n++) fn.quantize_row_q_dot(cx[n], xrow[n], 64);
    for (int r = 0; r < R; r++) fn.dequantize_row_q(row[r], cd[r], 64);
    for (int n = 0; n < NC; n++)
        for (int r = 0; r < R; r++) fn.vec_dot_q(64, &cy[n][r], row[r], xrow[n]);
    snprintf(shape, sizeof shape, "[%d, %d]", R, 2 * B);
    dump("craft_q", cw, (size_t)R * 2 * B, "u8", shape);
    snprintf(shape, sizeof shape, "[%d, 64]", R);
    dump("craft_dequant", cd, sizeof cd, "f32", shape);
    snprintf(shape, sizeof shape, "[%d, 64]", NC);
    dump("craft_x_f32", cx, sizeof cx, "f32", shape);
    snprintf(shape, sizeof shape, "[%d, %d]", NC, 2 * XB);
    dump("craft_x_q", cxq, (size_t)NC * 2 * XB, "u8", shape);
    snprintf(shape, sizeof shape, "[%d, %d]", NC, R);
    dump("craft_y", cy, sizeof cy, "f32", shape);

    fprintf(g_manifest, "\n}\n");
    fclose(g_manifest);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s outdir\n", argv[0]); return 2; }
    g_out = argv[1];
    { /* ggml_fp16_to_fp32 reads a table ggml_init builds: without it every d reads 0 */
        struct ggml_init_params ip = {1 << 20, NULL, false};
        ggml_free(ggml_init(ip));
    }
    return one_type(GGML_TYPE_Q4_1, "q41", 0, 1, 0x100) || one_type(GGML_TYPE_Q5_0, "q50", 1, 0, 0x200) ||
           one_type(GGML_TYPE_Q5_1, "q51", 1, 1, 0x300);
}
