/*
 * gen_golden_q8_0w.c — generates the Q8_0-weight fixtures in tests/golden/ (q8w_*.bin, q8w_manifest.json)
 * from the REFERENCE CPU path, compiled out of tree against the reference's ggml.c with
 * -march=x86-64-v3, so that ggml_vec_dot_q8_0_q8_0 and quantize_row_q8_0 run their AVX2 branches
 * (ggml.c:3231-3320, 1192-1275):
 *
 *   gcc -O2 -std=c11 -w -I$REF -march=x86-64-v3 -o gen_golden_q8_0w \
 *       tests/golden/gen_golden_q8_0w.c $REF/ggml.c -lm -lpthread
 *   ./gen_golden_q8_0w tests/golden
 *
 * Only this source and its output are committed.  The functions are reached through
 * ggml_internal_get_quantize_fn(GGML_TYPE_Q8_0).  Inputs come from a splitmix64 + Box-Muller generator
 * of its own, so they are reproducible without the reference.  The manifest has the format
 * tests/golden_io.py reads (variant "q8w").
 *
 * Per K in {64, 2304, 4160} (M = 24 weight rows, N = 3 activation rows; N = 1 is row 0):
 *   w<K>_q8_0     quantize_row_q8_0 of N(0, 0.02) rows             u8  [M, 34 K / 32]
 *   w<K>_dequant  dequantize_row_q8_0 of the first 8 rows          f32 [8, K]
 *   x<K>_f32      N(0, 1) activations                              f32 [N, K]
 *   x<K>_q8_0     quantize_row_q8_0 of them                        u8  [N, 34 K / 32]
 *   y<K>_vec_dot  ggml_vec_dot_q8_0_q8_0, AVX2                     f32 [N, M]
 * and crafted weight rows for K = 64 (two blocks per row, written byte by byte):
 *   craft_q8_0    u8 [R, 68]      craft_dequant  f32 [R, 64]
 *   craft_x_f32   f32 [NC, 64]    craft_x_q8_0   u8 [NC, 68]     craft_y  f32 [NC, R]
 *   rows: 0 all -128; 1 all +127; 2 alternating +-127; 3 d = 0 (block 0) and d = -0 (block 1);
 *         4 subnormal d (fp16 bits 0x0001 and 0x83FF); 5 -128 / +127 mixed with random bytes; 6 random bytes
 *   x:    0 N(0, 1); 1 alternating +-amax (every q = +-127); 2 all +amax; 3 all zero
 */
#include "ggml.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char *g_out;
static FILE *g_manifest;
static int g_first = 1;

static void dump(const char *name, const void *p, size_t n, const char *dtype, const char *shape) {
    char path[1024];
    snprintf(path, sizeof path, "%s/q8w_%s.bin", g_out, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path); exit(1); }
    fclose(f);
    fprintf(g_manifest, "%s    \"q8w_%s\": {\"file\": \"q8w_%s.bin\", \"bytes\": %zu, \"dtype\": \"%s\", \"shape\": %s}",
            g_first ? "" : ",\n", name, name, n, dtype, shape);
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

static void put_block(uint8_t *blk, uint16_t dbits, const int8_t *qs) {
    memcpy(blk, &dbits, 2);
    memcpy(blk + 2, qs, 32);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s outdir\n", argv[0]); return 2; }
    g_out = argv[1];
    { /* ggml_fp16_to_fp32 reads a table ggml_init builds: without it every d reads 0 */
        struct ggml_init_params ip = {1 << 20, NULL, false};
        ggml_free(ggml_init(ip));
    }
    const quantize_fns_t fn = ggml_internal_get_quantize_fn(GGML_TYPE_Q8_0);
    char mpath[1024];
    snprintf(mpath, sizeof mpath, "%s/q8w_manifest.json", g_out);
    g_manifest = fopen(mpath, "w");
    if (!g_manifest) { perror(mpath); return 1; }
    fprintf(g_manifest, "{\n");
    char name[64], shape[128];

    const int Ks[3] = {64, 2304, 4160};
    for (int ki = 0; ki < 3; ki++) {
        const int K = Ks[ki], M = 24, N = 3, nb = K / 32, DR = 8;
        float *wf = malloc((size_t)M * K * 4), *x = malloc((size_t)N * K * 4), *wd = malloc((size_t)DR * K * 4);
        uint8_t *wq = calloc((size_t)M * nb, 34), *xq = calloc((size_t)N * nb, 34);
        float y[3 * 24];
        fill_gaussian(wf, (size_t)M * K, 0x805EED00ull + K, 0.0f, 0.02f);
        fill_gaussian(x, (size_t)N * K, 0x805EED10ull + K, 0.0f, 1.0f);
        for (int m = 0; m < M; m++) fn.quantize_row_q(wf + (size_t)m * K, wq + (size_t)m * nb * 34, K);
        for (int n = 0; n < N; n++) fn.quantize_row_q_dot(x + (size_t)n * K, xq + (size_t)n * nb * 34, K);
        for (int m = 0; m < DR; m++) fn.dequantize_row_q(wq + (size_t)m * nb * 34, wd + (size_t)m * K, K);
        for (int n = 0; n < N; n++)
            for (int m = 0; m < M; m++)
                fn.vec_dot_q(K, &y[n * M + m], wq + (size_t)m * nb * 34, xq + (size_t)n * nb * 34);
        snprintf(name, sizeof name, "w%d_q8_0", K);
        snprintf(shape, sizeof shape, "[%d, %d]", M, nb * 34);
        dump(name, wq, (size_t)M * nb * 34, "u8", shape);
        snprintf(name, sizeof name, "w%d_dequant", K);
        snprintf(shape, sizeof shape, "[%d, %d]", DR, K);
        dump(name, wd, (size_t)DR * K * 4, "f32", shape);
        snprintf(name, sizeof name, "x%d_f32", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, K);
        dump(name, x, (size_t)N * K * 4, "f32", shape);
        snprintf(name, sizeof name, "x%d_q8_0", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, nb * 34);
        dump(name, xq, (size_t)N * nb * 34, "u8", shape);
        snprintf(name, sizeof name, "y%d_vec_dot", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, M);
        dump(name, y, (size_t)N * M * 4, "f32", shape);
        free(wf); free(x); free(wd); free(wq); free(xq);
    }

    /* crafted weight rows, K = 64 */
    enum { R = 7, NC = 4 };
    static uint8_t cw[R][68], cxq[NC][68];
    static float cx[NC][64], cd[R][64], cy[NC][R];
    int8_t qs[32];
    uint64_t s = 0x805EEDC0ull;
    const uint16_t d_a = ggml_fp32_to_fp16(0.0123f), d_b = ggml_fp32_to_fp16(-0.75f);
    memset(qs, -128, 32);
    put_block(cw[0], d_a, qs); put_block(cw[0] + 34, d_b, qs);
    memset(qs, 127, 32);
    put_block(cw[1], d_a, qs); put_block(cw[1] + 34, d_b, qs);
    for (int j = 0; j < 32; j++) qs[j] = (j & 1) ? -127 : 127;
    put_block(cw[2], d_a, qs);
    for (int j = 0; j < 32; j++) qs[j] = (j & 1) ? 127 : -127;
    put_block(cw[2] + 34, d_b, qs);
    for (int j = 0; j < 32; j++) qs[j] = (int8_t)(splitmix64(&s) & 0xFF);
    put_block(cw[3], 0x0000, qs); put_block(cw[3] + 34, 0x8000, qs);
    for (int j = 0; j < 32; j++) qs[j] = (int8_t)(splitmix64(&s) & 0xFF);
    put_block(cw[4], 0x0001, qs); put_block(cw[4] + 34, 0x83FF, qs);
    for (int j = 0; j < 32; j++) qs[j] = (j % 3 == 0) ? -128 : ((j % 3 == 1) ? 127 : (int8_t)(splitmix64(&s) & 0xFF));
    put_block(cw[5], d_b, qs);
    for (int j = 0; j < 32; j++) qs[j] = (j % 5 == 0) ? 127 : ((j % 5 == 2) ? -128 : (int8_t)(splitmix64(&s) & 0xFF));
    put_block(cw[5] + 34, d_a, qs);
    for (int b = 0; b < 2; b++) {
        for (int j = 0; j < 32; j++) qs[j] = (int8_t)(splitmix64(&s) & 0xFF);
        put_block(cw[6] + 34 * b, ggml_fp32_to_fp16(b ? 0.004f : 3.5f), qs);
    }
    fill_gaussian(cx[0], 64, 0x805EEDC1ull, 0.0f, 1.0f);
    for (int j = 0; j < 64; j++) { cx[1][j] = (j & 1) ? -3.0f : 3.0f; cx[2][j] = 0.37f; cx[3][j] = 0.0f; }
    for (int n = 0; n < NC; n++) fn.quantize_row_q_dot(cx[n], cxq[n], 64);
    for (int r = 0; r < R; r++) fn.dequantize_row_q(cw[r], cd[r], 64);
    for (int n = 0; n < NC; n++)
        for (int r = 0; r < R; r++) fn.vec_dot_q(64, &cy[n][r], cw[r], cxq[n]);
    snprintf(shape, sizeof shape, "[%d, 68]", R);
    dump("craft_q8_0", cw, sizeof cw, "u8", shape);
    snprintf(shape, sizeof shape, "[%d, 64]", R);
    dump("craft_dequant", cd, sizeof cd, "f32", shape);
    snprintf(shape, sizeof shape, "[%d, 64]", NC);
    dump("craft_x_f32", cx, sizeof cx, "f32", shape);
    snprintf(shape, sizeof shape, "[%d, 68]", NC);
    dump("craft_x_q8_0", cxq, sizeof cxq, "u8", shape);
    snprintf(shape, sizeof shape, "[%d, %d]", NC, R);
    dump("craft_y", cy, sizeof cy, "f32", shape);

    fprintf(g_manifest, "\n}\n");
    fclose(g_manifest);
    return 0;
}
