/*
 * gen_ops_golden.c — generates the layer-op fixtures in tests/golden/ (ops_*.bin, ops_manifest.json) from the
 * REFERENCE ggml CPU ops, compiled out of tree against the reference's ggml.c by oracle/Makefile (target
 * `golden_ops`, linked with oracle/_ref/ggml_avx2.o: -march=x86-64-v3, so ggml_vec_dot_f16 runs its AVX F16 loop
 * with FMA, ggml.c:2303).  It builds one-node graphs with the public API and runs them through
 * ggml_graph_compute on one thread: add, mul, scale, silu, rms_norm, diag_mask_inf, soft_max, rope (mode 0),
 * cpy (F32 -> F16 into a transposed view) and the F16 x F32 mul_mat.
 *
 * Only this source and its output are committed.  Inputs come from a splitmix64 + Box-Muller generator of
 * its own and from hand-made edge values, so they are reproducible without the reference.  The manifest has
 * the format tests/golden_io.py reads (variant "ops"); tests/test_ggml_ops_ref.py requires the numpy restatement
 * (tests/ggml_ops_ref.py) to reproduce every output bit for bit.
 *
 *   silu_table, exp_table   fp16(f / (1.0f + expf(-f))), fp16(expf(f)) for every fp16 pattern f, the formula of
 *                           ggml.c:4246-4254 with ggml_fp32_to_fp16 and this process's expf      u16 [65536]
 *                           (before writing: ggml_silu over all 65,536 fp16 values returns exactly the silu table)
 *   silu_x / silu_y         every fp16 exponent, +-0, |x| > 65504, fp16-subnormal magnitudes        f32 [n]
 *   add_a / add_b / add_y, scale_x / scale_v / scale_y                                            f32 [257]
 *   mul_a [3,5,6], mul_b1 [1,1,6] -> mul_y1, mul_b5 [1,5,6] -> mul_y5                              f32
 *   mask_x [2,3,9] -> mask_y0 (n_past 0), mask_y5 (n_past 5)                                       f32
 *   rms<n>_x / rms<n>_y     n = 6, 256, 4100; 3 rows: N(0,1), magnitudes spread over 2^+-20, tiny   f32 [3,n]
 *   sm<n>_x / sm<n>_y       n = 1, 65, 700; 4 rows: N(0,4); with -inf entries; differences below the fp16
 *                           subnormal step and exact fp16 rounding ties of x - max; differences beyond -65504
 *   rope<d>_<p>_x / _y      ne0 16, 2 heads, 3 tokens, n_dims d = 16, 8, n_past p = 0, 37           f32 [3,2,16]
 *   rope<d>_<p>_cos / _sin  the (cos, sin) of the run: theta from (float)p times powf(10000.0, -2.0f/d) per
 *                           pair, cosf / sinf of this process                                       f32 [3,8]
 *   cpy_x [2,5,7] f32 -> cpy_y: the F16 target [2,7,5] written through its transposed view          u16
 *   mm<K>_x [3,K] f16, mm<K>_y [5,K] f32 -> mm<K>_d [5,3], K = 1, 31, 32, 33, 40, 128, 500
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
    snprintf(path, sizeof path, "%s/ops_%s.bin", g_out, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { perror(path); exit(1); }
    fclose(f);
    fprintf(g_manifest, "%s    \"ops_%s\": {\"file\": \"ops_%s.bin\", \"bytes\": %zu, \"dtype\": \"%s\", \"shape\": %s}",
            g_first ? "" : ",\n", name, name, n, dtype, shape);
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
        const double u2 = (double)(splitmix64(&s) >> 11) / 9007199254740992.0;           /* [0, 1) */
        const double r = sqrt(-2.0 * log(u1));
        dst[i] = stdv * (float)(r * cos(6.283185307179586 * u2));
        if (i + 1 < n) dst[i + 1] = stdv * (float)(r * sin(6.283185307179586 * u2));
    }
}

static struct ggml_context *g_ctx;

static struct ggml_tensor *f32_tensor(const float *v, int64_t ne0, int64_t ne1, int64_t ne2) {
    struct ggml_tensor *t = ggml_new_tensor_3d(g_ctx, GGML_TYPE_F32, ne0, ne1, ne2);
    memcpy(t->data, v, ggml_nbytes(t));
    return t;
}

static void compute(struct ggml_tensor *out) {
    struct ggml_cgraph gf = ggml_build_forward(out);
    gf.n_threads = 1;
    ggml_graph_compute(g_ctx, &gf);
}

static uint32_t f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static void do_tables(void) {
    static uint16_t silu[65536], ex[65536];
    static float all[65536];
    for (int i = 0; i < 65536; i++) {
        const float f = ggml_fp16_to_fp32((ggml_fp16_t)i);
        silu[i] = ggml_fp32_to_fp16(f / (1.0f + expf(-f)));
        ex[i] = ggml_fp32_to_fp16(expf(f));
        all[i] = f;
    }
    /* the reference's own op over every fp16 value gives the table's entries (NaN inputs aside: the op's
     * conversion of the f32 NaN picks the quieted pattern's entry) */
    struct ggml_tensor *y = ggml_silu(g_ctx, f32_tensor(all, 65536, 1, 1));
    compute(y);
    for (int i = 0; i < 65536; i++) {
        if (all[i] != all[i]) continue;
        if (f32_bits(((float *)y->data)[i]) != f32_bits(ggml_fp16_to_fp32(silu[i]))) {
            fprintf(stderr, "ggml_silu(fp16 %#x) is not the table entry\n", i);
            exit(1);
        }
    }
    dump("silu_table", silu, sizeof silu, "u16", "[65536]");
    dump("exp_table", ex, sizeof ex, "u16", "[65536]");
}

static void do_silu(void) {
    float x[512];
    int n = 0;
    for (int e = -26; e <= 17; e++)                       /* every fp16 exponent (-14..15), below and above */
        for (int k = 0; k < 4; k++) {
            const float m = k == 0 ? 1.0f : k == 1 ? 1.37f : k == 2 ? 1.0004883f /* 1 + 2^-11: a tie */ : 1.9997f;
            x[n++] = ldexpf(m, e);
            x[n++] = -ldexpf(m, e);
        }
    const float extra[] = {0.0f, -0.0f, 65504.0f, -65504.0f, 65519.9f, 65520.0f, -65520.0f, 70000.0f, -70000.0f, 1e30f,
                           -1e30f, 5.9604645e-8f, -5.9604645e-8f, 1.7881393e-7f, 6.0975552e-5f, -6.0975552e-5f,
                           2.9802322e-8f, -2.9802322e-8f, 2.9802326e-8f, 1e-10f, -1e-10f, 1e-40f, 3.3f, -3.3f, 11.0f, -11.0f,
                           20.0f, -20.0f};
    for (size_t i = 0; i < sizeof extra / sizeof extra[0]; i++) x[n++] = extra[i];
    struct ggml_tensor *y = ggml_silu(g_ctx, f32_tensor(x, n, 1, 1));
    compute(y);
    char shape[64];
    snprintf(shape, sizeof shape, "[%d]", n);
    dump("silu_x", x, (size_t)n * 4, "f32", shape);
    dump("silu_y", y->data, (size_t)n * 4, "f32", shape);
}

static void do_elementwise(void) {
    enum { N = 257 };
    float a[N], b[N];
    fill_gaussian(a, N, 0x0A5EED01ull, 1.0f);
    fill_gaussian(b, N, 0x0A5EED02ull, 3.0f);
    struct ggml_tensor *y = ggml_add(g_ctx, f32_tensor(a, N, 1, 1), f32_tensor(b, N, 1, 1));
    compute(y);
    dump("add_a", a, sizeof a, "f32", "[257]");
    dump("add_b", b, sizeof b, "f32", "[257]");
    dump("add_y", y->data, sizeof a, "f32", "[257]");
    const float v = 1.0f / sqrtf(128.0f);
    y = ggml_scale(g_ctx, f32_tensor(b, N, 1, 1), ggml_new_f32(g_ctx, v));
    compute(y);
    dump("scale_x", b, sizeof b, "f32", "[257]");
    dump("scale_v", &v, 4, "f32", "[1]");
    dump("scale_y", y->data, sizeof b, "f32", "[257]");

    float ma[3 * 5 * 6], mb[5 * 6];
    fill_gaussian(ma, 90, 0x0A5EED03ull, 1.0f);
    fill_gaussian(mb, 30, 0x0A5EED04ull, 1.0f);
    dump("mul_a", ma, sizeof ma, "f32", "[3, 5, 6]");
    y = ggml_mul(g_ctx, f32_tensor(ma, 6, 5, 3), f32_tensor(mb, 6, 1, 1));
    compute(y);
    dump("mul_b1", mb, 6 * 4, "f32", "[1, 1, 6]");
    dump("mul_y1", y->data, sizeof ma, "f32", "[3, 5, 6]");
    y = ggml_mul(g_ctx, f32_tensor(ma, 6, 5, 3), f32_tensor(mb, 6, 5, 1));
    compute(y);
    dump("mul_b5", mb, sizeof mb, "f32", "[1, 5, 6]");
    dump("mul_y5", y->data, sizeof ma, "f32", "[3, 5, 6]");

    float mx[2 * 3 * 9];
    fill_gaussian(mx, 54, 0x0A5EED05ull, 1.0f);
    dump("mask_x", mx, sizeof mx, "f32", "[2, 3, 9]");
    y = ggml_diag_mask_inf(g_ctx, f32_tensor(mx, 9, 3, 2), 0);
    compute(y);
    dump("mask_y0", y->data, sizeof mx, "f32", "[2, 3, 9]");
    y = ggml_diag_mask_inf(g_ctx, f32_tensor(mx, 9, 3, 2), 5);
    compute(y);
    dump("mask_y5", y->data, sizeof mx, "f32", "[2, 3, 9]");
}

static void do_rms_norm(void) {
    const int ns[3] = {6, 256, 4100};
    for (int k = 0; k < 3; k++) {
        const int n = ns[k];
        float *x = malloc((size_t)3 * n * 4);
        fill_gaussian(x, (size_t)3 * n, 0x0B5EED00ull + n, 1.0f);
        uint64_t s = 0x0B5EED77ull + n;
        for (int i = 0; i < n; i++) {
            x[n + i] = ldexpf(x[n + i], (int)(splitmix64(&s) % 41) - 20);      /* row 1: spread over 2^+-20 */
            x[2 * n + i] *= 1e-4f;                                            /* row 2: mean near eps */
        }
        struct ggml_tensor *y = ggml_rms_norm(g_ctx, f32_tensor(x, n, 3, 1));
        compute(y);
        char name[64], shape[64];
        snprintf(shape, sizeof shape, "[3, %d]", n);
        snprintf(name, sizeof name, "rms%d_x", n);
        dump(name, x, (size_t)3 * n * 4, "f32", shape);
        snprintf(name, sizeof name, "rms%d_y", n);
        dump(name, y->data, (size_t)3 * n * 4, "f32", shape);
        free(x);
    }
}

static void do_soft_max(void) {
    const int ns[3] = {1, 65, 700};
    /* x - max with max = 0: exact fp16 rounding ties (1 + 2^-11, 1 + 3 2^-11, 2^-25: between 0 and the smallest
     * subnormal, 3 2^-25), differences below the fp16 subnormal step 2^-24 */
    const float fine[] = {-1.00048828125f, -1.00146484375f, -2.98023223876953125e-8f, -8.94069671630859375e-8f, -1e-9f,
                          -3e-8f, -2.9802326e-8f, -5.9604645e-8f, -6.1e-8f, -1e-12f, -1.0f, -0.5f};
    /* x - max with max = 10: beyond -65504 (65520 is the boundary to inf) */
    const float far[] = {-70000.0f, -65510.0f, -65509.9f, -65494.0f, -65493.9f, -1e6f, -3e38f, -65525.0f, -30000.0f, -11.0f};
    for (int k = 0; k < 3; k++) {
        const int n = ns[k];
        float *x = malloc((size_t)4 * n * 4);
        fill_gaussian(x, (size_t)4 * n, 0x0C5EED00ull + n, 4.0f);
        if (n > 1) {
            for (int i = 1; i < n; i += 3) x[n + i] = -INFINITY;                   /* row 1 */
            for (int i = 0; i < n; i++)                                            /* row 2 */
                x[2 * n + i] = i == 3 ? 0.0f : fine[i % (int)(sizeof fine / sizeof fine[0])];
            for (int i = 0; i < n; i++)                                            /* row 3 */
                x[3 * n + i] = i == 5 ? 10.0f : far[i % (int)(sizeof far / sizeof far[0])];
        } else {
            x[2] = 0.0f;
            x[3] = 1e5f;
        }
        struct ggml_tensor *y = ggml_soft_max(g_ctx, f32_tensor(x, n, 4, 1));
        compute(y);
        char name[64], shape[64];
        snprintf(shape, sizeof shape, "[4, %d]", n);
        snprintf(name, sizeof name, "sm%d_x", n);
        dump(name, x, (size_t)4 * n * 4, "f32", shape);
        snprintf(name, sizeof name, "sm%d_y", n);
        dump(name, y->data, (size_t)4 * n * 4, "f32", shape);
        free(x);
    }
}

static void do_rope(void) {
    enum { NE0 = 16, NH = 2, NT = 3 };
    float x[NT * NH * NE0];
    fill_gaussian(x, NT * NH * NE0, 0x0D5EED00ull, 2.0f);
    const int dims[2] = {16, 8}, pasts[2] = {0, 37};
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const int n_dims = dims[a], n_past = pasts[b];
            struct ggml_tensor *y = ggml_rope(g_ctx, f32_tensor(x, NE0, NH, NT), n_past, n_dims, 0, 0);
            compute(y);
            float c[NT * NE0 / 2], s[NT * NE0 / 2];
            const float theta_scale = powf(10000.0, -2.0f / n_dims);
            for (int t = 0; t < NT; t++) {
                float theta = (float)(n_past + t);
                for (int j = 0; j < NE0 / 2; j++) {
                    c[t * NE0 / 2 + j] = cosf(theta);
                    s[t * NE0 / 2 + j] = sinf(theta);
                    theta *= theta_scale;
                }
            }
            char name[64];
            snprintf(name, sizeof name, "rope%d_%d_x", n_dims, n_past);
            dump(name, x, sizeof x, "f32", "[3, 2, 16]");
            snprintf(name, sizeof name, "rope%d_%d_y", n_dims, n_past);
            dump(name, y->data, sizeof x, "f32", "[3, 2, 16]");
            snprintf(name, sizeof name, "rope%d_%d_cos", n_dims, n_past);
            dump(name, c, sizeof c, "f32", "[3, 8]");
            snprintf(name, sizeof name, "rope%d_%d_sin", n_dims, n_past);
            dump(name, s, sizeof s, "f32", "[3, 8]");
        }
}

static void do_cpy(void) {
    float x[2 * 5 * 7];
    fill_gaussian(x, 70, 0x0E5EED00ull, 1.0f);
    x[0] = 1.00048828125f;            /* fp16 ties and the overflow boundary */
    x[1] = 1.00146484375f;
    x[2] = 65519.9f;
    x[3] = 65520.0f;
    x[4] = -2.98023223876953125e-8f;
    x[5] = 1e-10f;
    struct ggml_tensor *base = ggml_new_tensor_3d(g_ctx, GGML_TYPE_F16, 5, 7, 2);
    memset(base->data, 0, ggml_nbytes(base));
    struct ggml_tensor *y = ggml_cpy(g_ctx, f32_tensor(x, 7, 5, 2), ggml_transpose(g_ctx, base));
    compute(y);
    dump("cpy_x", x, sizeof x, "f32", "[2, 5, 7]");
    dump("cpy_y", base->data, ggml_nbytes(base), "u16", "[2, 7, 5]");
}

static void do_mul_mat(void) {
    const int Ks[7] = {1, 31, 32, 33, 40, 128, 500};
    for (int k = 0; k < 7; k++) {
        const int K = Ks[k];
        float xf[3 * 500], yf[5 * 500];
        fill_gaussian(xf, (size_t)3 * K, 0x0F5EED00ull + K, 0.5f);
        fill_gaussian(yf, (size_t)5 * K, 0x0F5EED80ull + K, 1.0f);
        struct ggml_tensor *x = ggml_new_tensor_2d(g_ctx, GGML_TYPE_F16, K, 3);
        for (int i = 0; i < 3 * K; i++) ((ggml_fp16_t *)x->data)[i] = ggml_fp32_to_fp16(xf[i]);
        struct ggml_tensor *d = ggml_mul_mat(g_ctx, x, f32_tensor(yf, K, 5, 1));
        compute(d);
        char name[64], shape[64];
        snprintf(name, sizeof name, "mm%d_x", K);
        snprintf(shape, sizeof shape, "[3, %d]", K);
        dump(name, x->data, (size_t)3 * K * 2, "u16", shape);
        snprintf(name, sizeof name, "mm%d_y", K);
        snprintf(shape, sizeof shape, "[5, %d]", K);
        dump(name, yf, (size_t)5 * K * 4, "f32", shape);
        snprintf(name, sizeof name, "mm%d_d", K);
        dump(name, d->data, 15 * 4, "f32", "[5, 3]");
    }
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s outdir\n", argv[0]); return 2; }
    g_out = argv[1];
    char mpath[1024];
    snprintf(mpath, sizeof mpath, "%s/ops_manifest.json", g_out);
    g_manifest = fopen(mpath, "w");
    if (!g_manifest) { perror(mpath); return 1; }
    fprintf(g_manifest, "{\n");
    struct ggml_init_params ip = {(size_t)64 << 20, NULL, false};
    g_ctx = ggml_init(ip);
    do_tables();
    do_silu();
    do_elementwise();
    do_rms_norm();
    do_soft_max();
    do_rope();
    do_cpy();
    do_mul_mat();
    ggml_free(g_ctx);
    fprintf(g_manifest, "\n}\n");
    fclose(g_manifest);
    return 0;
}
