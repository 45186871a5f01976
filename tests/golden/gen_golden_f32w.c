/*
 * gen_golden_f32w.c — generates the F32-weight fixtures in tests/golden/ (f32w_*.bin, f32w_manifest.json) from the
 * REFERENCE CPU path: the real ggml_mul_mat + ggml_graph_compute with an F32 src0
 * (ggml_compute_forward_mul_mat_f32, ggml.c:10855 -> ggml_vec_dot_f32, ggml.c:2266), compiled out of tree against the
 * reference's ggml.c with -march=x86-64-v3 so that the AVX2 + FMA schedule runs (GGML_F32_STEP 32, GGML_F32_EPR 8):
 *
 *   gcc -O2 -std=c11 -w -I$REF -march=x86-64-v3 -o gen_golden_f32w tests/golden/gen_golden_f32w.c $REF/ggml.c \
 *       -lm -lpthread
 *   ./gen_golden_f32w tests/golden
 *
 * Only this source and its output are committed.  Inputs come from a splitmix64 + Box-Muller generator of its own, so
 * they are reproducible without the reference.  The manifest has the format tests/golden_io.py reads (variant "f32w").
 *
 * Per K (32, 288, 1056; M = 24 weight rows, N = 3 activation rows; every K a multiple of 32, so the scalar leftover
 * loop never runs):
 *   w<K>_f32        N(0, 0.5) weights, magnitudes spread over 2^+-20; row 0 holds only +-0 and one subnormal weight
 *                   2^-130 against x = 2^20; rows 1 and 2 hold +-0, subnormals and 2^-126 among ordinary values
 *                                                                                       f32 [M, K]
 *   x<K>_f32        N(0, 1) activations, a few of large magnitude                       f32 [N, K]
 *   y<K>_t1 / _t4   dst of ggml_mul_mat on 1 and on 4 threads                           f32 [N, M]
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

static void dump(const char *name, const void *p, size_t n, const char *shape) {
    char path[1024];
    snprintf(path, sizeof path, "%s/f32w_%s.bin", g_out, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path); exit(1); }
    fclose(f);
    fprintf(g_manifest, "%s    \"f32w_%s\": {\"file\": \"f32w_%s.bin\", \"bytes\": %zu, \"dtype\": \"f32\", \"shape\": %s}",
            g_first ? "" : ",\n", name, name, n, shape);
    g_first = 0;
}

static uint64_t splitmix64(uint64_t *s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void fill_gaussian(float *dst, size_t n, uint64_t seed, float stdv) {
    uint64_t s = seed;
    for (size_t i = 0; i < n; i += 2) {
        const double u1 = ((double)(splitmix64(&s) >> 11) + 1.0) / 9007199254740992.0;   /* (0, 1] */
        const double u2 = (double)(splitmix64(&s) >> 11) / 9007199254740992.0;
        const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
        dst[i] = (float)(stdv * r * cos(a));
        if (i + 1 < n) dst[i + 1] = (float)(stdv * r * sin(a));
    }
}

static void run(int K, int M, int N, const float *w, const float *x, int threads, float *y) {
    struct ggml_init_params ip = {(size_t)64 << 20, NULL, 0};
    struct ggml_context *ctx = ggml_init(ip);
    struct ggml_tensor *a = ggml_new_tensor_2d(ctx, GGML_TYPE_F32, K, M);
    struct ggml_tensor *b = ggml_new_tensor_2d(ctx, GGML_TYPE_F32, K, N);
    memcpy(a->data, w, sizeof(float) * (size_t)M * K);
    memcpy(b->data, x, sizeof(float) * (size_t)N * K);
    struct ggml_tensor *c = ggml_mul_mat(ctx, a, b);
    struct ggml_cgraph gf = ggml_build_forward(c);
    gf.n_threads = threads;
    ggml_graph_compute(ctx, &gf);
    memcpy(y, c->data, sizeof(float) * (size_t)N * M);
    ggml_free(ctx);
}

int main(int argc, char **argv) {
    g_out = argc > 1 ? argv[1] : ".";
    char path[1024];
    snprintf(path, sizeof path, "%s/f32w_manifest.json", g_out);
    g_manifest = fopen(path, "w");
    if (!g_manifest) { perror(path); return 1; }
    fprintf(g_manifest, "{\n");
    const int Ks[3] = {32, 288, 1056}, M = 24, N = 3;
    for (int ki = 0; ki < 3; ki++) {
        const int K = Ks[ki];
        float *w = malloc(sizeof(float) * M * K), *x = malloc(sizeof(float) * N * K), *y = malloc(sizeof(float) * N * M);
        fill_gaussian(w, (size_t)M * K, 0xF32A0000u + K, 0.5f);
        fill_gaussian(x, (size_t)N * K, 0xF32B0000u + K, 1.0f);
        uint64_t s = 0xF32C0000u + K;
        for (int i = 0; i < M * K; i++) w[i] = ldexpf(w[i], (int)(splitmix64(&s) % 41) - 20);
        for (int i = 0; i < N * K; i += 37) x[i] = ldexpf(x[i], (int)(splitmix64(&s) % 31));
        const float pats[8] = {0.0f, -0.0f, ldexpf(1.0f, -130), -ldexpf(1.0f, -130), ldexpf(1.0f, -149), 1e-30f,
                               -3e-39f, ldexpf(1.0f, -126)};
        for (int r = 1; r <= 2; r++)
            for (int i = r; i < K; i += 3) w[r * K + i] = pats[(i / 3 + r) % 8];
        for (int i = 0; i < K; i++) w[i] = (i & 1) ? -0.0f : 0.0f;
        w[5] = ldexpf(1.0f, -130);
        for (int n = 0; n < N; n++) x[n * K + 5] = ldexpf(1.0f, 20);
        char name[64], shape[64];
        snprintf(name, sizeof name, "w%d_f32", K);
        snprintf(shape, sizeof shape, "[%d, %d]", M, K);
        dump(name, w, sizeof(float) * M * K, shape);
        snprintf(name, sizeof name, "x%d_f32", K);
        snprintf(shape, sizeof shape, "[%d, %d]", N, K);
        dump(name, x, sizeof(float) * N * K, shape);
        snprintf(shape, sizeof shape, "[%d, %d]", N, M);
        run(K, M, N, w, x, 1, y);
        snprintf(name, sizeof name, "y%d_t1", K);
        dump(name, y, sizeof(float) * N * M, shape);
        run(K, M, N, w, x, 4, y);
        snprintf(name, sizeof name, "y%d_t4", K);
        dump(name, y, sizeof(float) * N * M, shape);
        free(w), free(x), free(y);
    }
    fprintf(g_manifest, "\n}\n");
    fclose(g_manifest);
    return 0;
}
