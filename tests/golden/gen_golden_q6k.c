/*
 * gen_golden_q6k.c — generates the Q6_K fixtures in tests/golden/ (q6k_*.bin, q6k_manifest.json,
 * ggml_type_sizes.json) from the REFERENCE k-quants CPU path, compiled out of tree against the
 * reference's ggml.c and k_quants.c with k-quants on and -march=x86-64-v3, so that
 * ggml_vec_dot_q6_K_q8_K runs its AVX2 branch (k_quants.c:3484-3561):
 *
 *   gcc -O2 -std=c11 -w -I$REF -DGGML_USE_K_QUANTS -march=x86-64-v3 -o gen_golden_q6k \
 *       tests/golden/gen_golden_q6k.c $REF/ggml.c $REF/k_quants.c -lm -lpthread
 *   ./gen_golden_q6k tests/golden
 *
 * Only this source and its output are committed.  Inputs come from a splitmix64 + Box-Muller
 * generator of its own, so they are reproducible without the reference.  The manifest has the format
 * tests/golden_io.py reads (variant "q6k").
 *
 * Per K in {256, 2304, 4096} (M = 24 weight rows, N = 3 activation rows; N = 1 is row 0):
 *   w<K>_q6_K     quantize_row_q6_K of N(0, 0.02) rows             u8  [M, 210 K / 256]
 *   w<K>_dequant  dequantize_row_q6_K of the first 8 rows          f32 [8, K]
 *   x<K>_f32      N(0, 1) activations                              f32 [N, K]
 *   x<K>_q8_K     quantize_row_q8_K of them                        u8  [N, 292 K / 256]
 *   y<K>_vec_dot  ggml_vec_dot_q6_K_q8_K, AVX2                     f32 [N, M]
 * and crafted activation blocks (one block of 256 per row):
 *   craft_f32 / craft_q8_K                                         f32 [R, 256] / u8 [R, 292]
 * The q8_K buffers are zeroed first: the reference leaves bsums of an all-zero block unwritten.
 */
#include "ggml.h"
#include "k_quants.h"

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
    snprintf(path, sizeof path, "%s/q6k_%s.bin", g_out, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path); exit(1); }
    fclose(f);
    fprintf(g_manifest, "%s    \"q6k_%s\": {\"file\": \"q6k_%s.bin\", \"bytes\": %zu, \"dtype\": \"%s\", \"shape\": %s}",
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

static void type_sizes(void) {
    static const char *names[GGML_TYPE_COUNT] = {"F32", "F16", "Q4_0", "Q4_1", "", "", "Q5_0", "Q5_1", "Q8_0", "Q8_1",
                                                 "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K", "I8", "I16", "I32"};
    char path[1024];
    snprintf(path, sizeof path, "%s/ggml_type_sizes.json", g_out);
    FILE *f = fopen(path, "w");
    if (!f) { perror(path); exit(1); }
    fprintf(f, "{");
    int first = 1;
    for (int t = 0; t < GGML_TYPE_COUNT; t++) {
        if (!names[t][0]) continue;          /* 4, 5: removed types, no table entry */
        fprintf(f, "%s\"%d\": {\"name\": \"%s\", \"size\": %zu, \"blck\": %d}", first ? "" : ", ", t, names[t],
                ggml_type_size((enum ggml_type)t), ggml_blck_size((enum ggml_type)t));
        first = 0;
    }
    fprintf(f, "}\n");
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s outdir\n", argv[0]); return 2; }
    g_out = argv[1];
    { /* ggml_fp16_to_fp32 reads a table ggml_init builds: without it every d reads 0 */
        struct ggml_init_params ip = {1 << 20, NULL, false};
        ggml_free(ggml_init(ip));
    }
    type_sizes();
    char mpath[1024];
    snprintf(mpath, sizeof mpath, "%s/q6k_manifest.json", g_out);
    g_manifest = fopen(mpath, "w");
    if (!g_manifest) { perror(mpath); return 1; }
    fprintf(g_manifest, "{\n");
    char name[64], shape[128];

    const int Ks[3] = {256, 2304, 4096};
    for (int ki = 0; ki < 3; ki++) {
        const int K = Ks[ki], M = 24, N = 3, nb = K / 256, DR = 8;
        float *wf = malloc((size_t)M * K * 4), *x = malloc((size_t)N * K * 4), *wd = malloc((size_t)DR * K * 4);
        uint8_t *wq = calloc((size_t)M * nb, 210), *xq = calloc((size_t)N * nb, 292);
        float y[3 * 24];
        fill_gaussian(wf, (size_t)M * K, 0x6B5EED00ull + K, 0.0f, 0.02f);
        fill_gaussian(x, (size_t)N * K, 0x6B5EED10ull + K, 0.0f, 1.0f);
        for (int m = 0; m < M; m++) quantize_row_q6_K(wf + (size_t)m * K, wq + (size_t)m * nb * 210, K);
        for (int n = 0; n < N; n++) quantize_row_q8_K(x + (size_t)n * K, xq + (size_t)n * nb * 292, K);
        for (int m = 0; m < DR; m++) dequantize_row_q6_K((const block_q6_K *)(wq + (size_t)m * nb * 210), wd + (size_t)m * K, K);
        for (int n = 0; n < N; n++)
            for (int m = 0; m < M; m++)
                ggml_vec_dot_q6_K_q8_K(K, &y[n * M + m], wq + (size_t)m * nb * 210, xq + (size_t)n * nb * 292);
        snprintf(name, sizeof name, "w%d_q6_K", K);
        snprintf(shape, sizeof shape, "[%d, %d]", M, nb * 210);
        dump(name, wq, (size_t)M * nb * 210, "u8", shape);
        snprintf(name, sizeof name, "w%d_dequant", K);
        snprintf(shape, sizeof shape, "[%d, %d]", DR, K);
        dump(name, wd, (size_t)DR * K * 4, "f32", shape);
        snprintf(name, sizeof name, "x%d_f32", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, K);
        dump(name, x, (size_t)N * K * 4, "f32", shape);
        snprintf(name, sizeof name, "x%d_q8_K", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, nb * 292);
        dump(name, xq, (size_t)N * nb * 292, "u8", shape);
        snprintf(name, sizeof name, "y%d_vec_dot", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, M);
        dump(name, y, (size_t)N * M * 4, "f32", shape);
        free(wf); free(x); free(wd); free(wq); free(xq);
    }

    /* crafted blocks; |x| is 0 or within [2^-100, 2^100] */
    enum { R = 12 };
    static float c[R][256];
    static uint8_t cq[R][292];
    memset(c, 0, sizeof c);
    memset(cq, 0, sizeof cq);
    /* 0: all zero.  1: +max before -max.  2: -max before +max (the later one maps to +128 -> 127) */
    fill_gaussian(c[1], 256, 0x6B5EED21ull, 0.0f, 0.5f);
    fill_gaussian(c[2], 256, 0x6B5EED22ull, 0.0f, 0.5f);
    for (int j = 0; j < 256; j++) {
        if (fabsf(c[1][j]) >= 2.0f) c[1][j] = 1.0f;
        if (fabsf(c[2][j]) >= 2.0f) c[2][j] = -1.0f;
    }
    c[1][5] = 2.0f;  c[1][9] = -2.0f;
    c[2][5] = -2.0f; c[2][9] = 2.0f;
    /* 3, 4: exact half-way products: amax = 128 gives iscale = -1 / +1, x = 0.5, 1.5, 2.5, ... of both signs */
    c[3][0] = 128.0f;
    c[4][0] = -128.0f;
    for (int j = 1; j < 256; j++) {
        const float v = (float)((j - 1) % 127) + 0.5f;
        c[3][j] = (j & 1) ? v : -v;
        c[4][j] = (j & 2) ? v : -v;
    }
    /* 5: the maximum last, a tie in |x| in front of it at lower magnitude; 6: all elements equal */
    for (int j = 0; j < 256; j++) { c[5][j] = (j & 1) ? 0.75f : -0.75f; c[6][j] = -3.0f; }
    c[5][255] = -1.0f;
    /* 7 .. 11: block maxima spread over 2^+-100 */
    fill_gaussian(c[7], 256, 0x6B5EED27ull, 0.0f, 1.0f);
    for (int j = 0; j < 256; j++) c[7][j] = ldexpf(c[7][j], 96);
    c[7][17] = -ldexpf(1.0f, 100);
    for (int j = 0; j < 256; j++) c[8][j] = (j % 3 == 0) ? 0.0f : ((j % 3 == 1) ? ldexpf(1.0f, -100) : -ldexpf(1.0f, -100));
    fill_gaussian(c[9], 256, 0x6B5EED29ull, 0.0f, 1.0f);
    for (int j = 0; j < 256; j++) c[9][j] = ldexpf(c[9][j], 60);
    fill_gaussian(c[10], 256, 0x6B5EED2Aull, 0.0f, 1.0f);
    for (int j = 0; j < 256; j++) c[10][j] = ldexpf(c[10][j], -60);
    fill_gaussian(c[11], 256, 0x6B5EED2Bull, 0.0f, 1.0f);
    for (int j = 0; j < 256; j++) c[11][j] = (j == 200) ? ldexpf(1.0f, 100) : ldexpf(c[11][j], -90);
    for (int r = 0; r < R; r++)
        for (int j = 0; j < 256; j++) {
            const float a = fabsf(c[r][j]);
            if (a != 0.0f && (a < ldexpf(1.0f, -100) || a > ldexpf(1.0f, 100))) c[r][j] = 0.0f;
        }
    for (int r = 0; r < R; r++) quantize_row_q8_K(c[r], cq[r], 256);
    snprintf(shape, sizeof shape, "[%d, 256]", R);
    dump("craft_f32", c, sizeof c, "f32", shape);
    snprintf(shape, sizeof shape, "[%d, 292]", R);
    dump("craft_q8_K", cq, sizeof cq, "u8", shape);

    fprintf(g_manifest, "\n}\n");
    fclose(g_manifest);
    return 0;
}
