/*
 * gen_golden_q23k.c — generates the Q3_K and Q2_K fixtures in tests/golden/ (q3k_*.bin, q3k_manifest.json,
 * q2k_*.bin, q2k_manifest.json) from the REFERENCE k-quants CPU path, compiled out of tree against the
 * reference's ggml.c and k_quants.c with k-quants on and -march=x86-64-v3, so that
 * ggml_vec_dot_q3_K_q8_K and ggml_vec_dot_q2_K_q8_K run their AVX2 branches (k_quants.c:1836-1938,
 * 1330-1394); -std=c11 keeps the compiler from contracting the Q2_K dequantizer's `dl * q - ml` into a fused
 * multiply-add:
 *
 *   gcc -O2 -std=c11 -w -I$REF -DGGML_USE_K_QUANTS -march=x86-64-v3 -o gen_golden_q23k \
 *       tests/golden/gen_golden_q23k.c $REF/ggml.c $REF/k_quants.c -lm -lpthread
 *   ./gen_golden_q23k tests/golden
 *
 * Only this source and its output are committed.  Inputs come from a splitmix64 + Box-Muller
 * generator of its own, so they are reproducible without the reference.  The manifests have the format
 * tests/golden_io.py reads (variants "q3k" and "q2k").
 *
 * Per type and K (256, 768, 4096; M = 24 weight rows, N = 3 activation rows):
 *   w<K>_q3_K / w<K>_q2_K  quantize_row_q3_K / quantize_row_q2_K of N(0, 0.02) rows   u8  [M, 110 | 84 K / 256]
 *   w<K>_dequant           dequantize_row_q3_K / _q2_K of the first 8 rows            f32 [8, K]
 *   x<K>_f32               N(0, 1) activations                                        f32 [N, K]
 *   x<K>_q8_K              quantize_row_q8_K of them                                  u8  [N, 292 K / 256]
 *   y<K>_vec_dot           ggml_vec_dot_q3_K_q8_K / _q2_K_q8_K, AVX2                  f32 [N, M]
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
static const char *g_variant;
static FILE *g_manifest;
static int g_first;

static void dump(const char *name, const void *p, size_t n, const char *dtype, const char *shape) {
    char path[1024];
    snprintf(path, sizeof path, "%s/%s_%s.bin", g_out, g_variant, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path); exit(1); }
    fclose(f);
    fprintf(g_manifest, "%s    \"%s_%s\": {\"file\": \"%s_%s.bin\", \"bytes\": %zu, \"dtype\": \"%s\", \"shape\": %s}",
            g_first ? "" : ",\n", g_variant, name, g_variant, name, n, dtype, shape);
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

/* one type: q3 = 1 Q3_K (110-byte blocks), q3 = 0 Q2_K (84-byte blocks) */
static void one_type(int q3, const int *Ks, int nK) {
    const int bs = q3 ? 110 : 84;
    const char *tname = q3 ? "q3_K" : "q2_K";
    char mpath[1024], name[64], shape[128];
    g_variant = q3 ? "q3k" : "q2k";
    g_first = 1;
    snprintf(mpath, sizeof mpath, "%s/%s_manifest.json", g_out, g_variant);
    g_manifest = fopen(mpath, "w");
    if (!g_manifest) { perror(mpath); exit(1); }
    fprintf(g_manifest, "{\n");
    for (int ki = 0; ki < nK; ki++) {
        const int K = Ks[ki], M = 24, N = 3, nb = K / 256, DR = 8;
        float *wf = malloc((size_t)M * K * 4), *x = malloc((size_t)N * K * 4), *wd = malloc((size_t)DR * K * 4);
        uint8_t *wq = calloc((size_t)M * nb, bs), *xq = calloc((size_t)N * nb, 292);
        float y[3 * 24];
        fill_gaussian(wf, (size_t)M * K, (q3 ? 0x3B5EED00ull : 0x2B5EED00ull) + K, 0.0f, 0.02f);
        fill_gaussian(x, (size_t)N * K, (q3 ? 0x3B5EED10ull : 0x2B5EED10ull) + K, 0.0f, 1.0f);
        for (int m = 0; m < M; m++) {
            if (q3) quantize_row_q3_K(wf + (size_t)m * K, wq + (size_t)m * nb * bs, K);
            else quantize_row_q2_K(wf + (size_t)m * K, wq + (size_t)m * nb * bs, K);
        }
        for (int n = 0; n < N; n++) quantize_row_q8_K(x + (size_t)n * K, xq + (size_t)n * nb * 292, K);
        for (int m = 0; m < DR; m++) {
            if (q3) dequantize_row_q3_K((const block_q3_K *)(wq + (size_t)m * nb * bs), wd + (size_t)m * K, K);
            else dequantize_row_q2_K((const block_q2_K *)(wq + (size_t)m * nb * bs), wd + (size_t)m * K, K);
        }
        for (int n = 0; n < N; n++)
            for (int m = 0; m < M; m++) {
                if (q3) ggml_vec_dot_q3_K_q8_K(K, &y[n * M + m], wq + (size_t)m * nb * bs, xq + (size_t)n * nb * 292);
                else ggml_vec_dot_q2_K_q8_K(K, &y[n * M + m], wq + (size_t)m * nb * bs, xq + (size_t)n * nb * 292);
            }
        snprintf(name, sizeof name, "w%d_%s", K, tname);
        snprintf(shape, sizeof shape, "[%d, %d]", M, nb * bs);
        dump(name, wq, (size_t)M * nb * bs, "u8", shape);
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
    fprintf(g_manifest, "\n}\n");
    fclose(g_manifest);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s outdir\n", argv[0]); return 2; }
    g_out = argv[1];
    { /* ggml_fp16_to_fp32 reads a table ggml_init builds: without it every d reads 0 */
        struct ggml_init_params ip = {1 << 20, NULL, false};
        ggml_free(ggml_init(ip));
    }
    const int Ks[3] = {256, 768, 4096};
    one_type(1, Ks, 3);
    one_type(0, Ks, 3);
    return 0;
}
