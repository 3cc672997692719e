/* Stand-alone program around oracle/va_oracle.c for tests/test_special_values_host.py: built with
 * -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all and run directly, it calls the oracle's float
 * entry points on the inputs the GPU test compares and exits 0 when none of them leaves defined C.
 *
 *   special_values_driver <calls> <results>
 *
 * <calls> is a sequence of records (tests/special_values_checks.py, record()): int64 op, int64 a[7], double p[2],
 * then the input arrays of the op, packed.  Every output is appended to <results>.
 * Op 10 is not the oracle's: it is the running mean's division-free quotient (div_by_uniform of va_point.hip),
 * three lines of C, next to the plain division it stands for. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int vao_gaussian_f32(const float *src, float *dst, int n, int h, int w, int c, double sigma);
void vao_bg_mean_u8(const uint8_t *frames, uint8_t *diff_out, double *mean, int64_t n_seen, int n, size_t px);
int vao_mean_any(const void *frames, int dtype, double *mean, int64_t n_seen, int n, size_t px);
int vao_welford_any(const void *frames, int dtype, double *mean, double *m2, int64_t n_seen, int n, size_t px);
void vao_welford_u8(const uint8_t *frames, double *mean, double *m2, int64_t n_seen, int n, size_t px);
void vao_bg_ema_f32(const float *frames, float *diff_out, float *bg, int64_t n_seen, float rate, int n, size_t px);
void vao_bg_ema_u8(const uint8_t *frames, uint8_t *diff_out, float *bg, int64_t n_seen, float rate, int n, size_t px);
void vao_bg_static_u8(const uint8_t *frames, uint8_t *diff_out, const double *bg, int n, size_t px);
int vao_resize_f32(const float *src, float *dst, int n, int sh, int sw, int c, int dh, int dw, int mode);

static FILE *in, *out;

static void *take(size_t bytes)
{
    void *p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, in) != bytes) {
        fprintf(stderr, "special_values_driver: short input\n");
        exit(3);
    }
    return p;
}
static void *room(size_t bytes)
{
    void *p = calloc(bytes ? bytes : 1, 1);
    if (!p)
        exit(3);
    return p;
}
static void give(void *p, size_t bytes)
{
    if (fwrite(p, 1, bytes, out) != bytes)
        exit(3);
    free(p);
}
static size_t element_size(int dtype) { return dtype == 0 ? 1 : dtype == 3 ? 2 : 4; }

static double div_by_uniform(double x, double d, double y)
{
    const double q = x * y;
    const double r = fma(-q, d, x);
    return fma(r, y, q);
}

int main(int argc, char **argv)
{
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) {
        fprintf(stderr, "usage: special_values_driver <calls> <results>\n");
        return 2;
    }
    int64_t a[8];
    double p[2];
    long calls = 0;
    while (fread(a, sizeof a, 1, in) == 1) {
        if (fread(p, sizeof p, 1, in) != 1)
            return 3;
        const int op = (int)a[0];
        int rc = 0;
        if (op == 1) {                                   /* n h w c; sigma */
            const size_t count = (size_t)(a[1] * a[2] * a[3] * a[4]);
            float *src = take(4 * count), *dst = room(4 * count);
            rc = vao_gaussian_f32(src, dst, (int)a[1], (int)a[2], (int)a[3], (int)a[4], p[0]);
            give(dst, 4 * count);
            free(src);
        } else if (op == 2 || op == 3) {                 /* n px n_seen want_diff; rate */
            const size_t n = (size_t)a[1], px = (size_t)a[2], es = op == 2 ? 4 : 1;
            void *fr = take(es * n * px);
            float *bg = take(4 * px);
            void *diff = a[4] ? room(es * n * px) : NULL;
            if (op == 2)
                vao_bg_ema_f32(fr, diff, bg, a[3], (float)p[0], (int)n, px);
            else
                vao_bg_ema_u8(fr, diff, bg, a[3], (float)p[0], (int)n, px);
            if (diff)
                give(diff, es * n * px);
            give(bg, 4 * px);
            free(fr);
        } else if (op == 4) {                            /* n px n_seen want_diff */
            const size_t n = (size_t)a[1], px = (size_t)a[2];
            uint8_t *fr = take(n * px);
            double *mean = take(8 * px);
            uint8_t *diff = a[4] ? room(n * px) : NULL;
            vao_bg_mean_u8(fr, diff, mean, a[3], (int)n, px);
            if (diff)
                give(diff, n * px);
            give(mean, 8 * px);
            free(fr);
        } else if (op == 5 || op == 6 || op == 7) {      /* n px n_seen dtype */
            const size_t n = (size_t)a[1], px = (size_t)a[2];
            const int dtype = op == 5 ? 0 : (int)a[4];
            void *fr = take(element_size(dtype) * n * px);
            double *mean = take(8 * px), *m2 = op == 7 ? NULL : take(8 * px);
            if (op == 5)
                vao_welford_u8(fr, mean, m2, a[3], (int)n, px);
            else if (op == 6)
                rc = vao_welford_any(fr, dtype, mean, m2, a[3], (int)n, px);
            else
                rc = vao_mean_any(fr, dtype, mean, a[3], (int)n, px);
            give(mean, 8 * px);
            if (m2)
                give(m2, 8 * px);
            free(fr);
        } else if (op == 8) {                            /* n px */
            const size_t n = (size_t)a[1], px = (size_t)a[2];
            uint8_t *fr = take(n * px), *diff = room(n * px);
            double *bg = take(8 * px);
            vao_bg_static_u8(fr, diff, bg, (int)n, px);
            give(diff, n * px);
            free(bg);
            free(fr);
        } else if (op == 9) {                            /* n sh sw c dh dw mode */
            const size_t ni = (size_t)(a[1] * a[2] * a[3] * a[4]), no = (size_t)(a[1] * a[5] * a[6] * a[4]);
            float *src = take(4 * ni), *dst = room(4 * no);
            rc = vao_resize_f32(src, dst, (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7]);
            give(dst, 4 * no);
            free(src);
        } else if (op == 10) {                           /* count: x[count], d[count] -> model[count], plain[count] */
            const size_t count = (size_t)a[1];
            double *x = take(8 * count), *d = take(8 * count), *model = room(8 * count), *plain = room(8 * count);
            for (size_t i = 0; i < count; i++) {
                const double y = 1.0 / d[i];
                model[i] = div_by_uniform(x[i], d[i], y);
                plain[i] = x[i] / d[i];
            }
            give(model, 8 * count);
            give(plain, 8 * count);
            free(x);
            free(d);
        } else {
            fprintf(stderr, "special_values_driver: unknown op %d\n", op);
            return 2;
        }
        if (rc) {
            fprintf(stderr, "special_values_driver: op %d of call %ld returned %d\n", op, calls, rc);
            return 4;
        }
        calls++;
    }
    if (fclose(out))
        return 3;
    printf("%ld calls\n", calls);
    return 0;
}
