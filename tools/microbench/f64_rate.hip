// micro-benchmark: issue rate of the float64 VALU ops of the running-mean kernel on gfx950
// build: hipcc --offload-arch=gfx950 -O3 f64_rate.hip -o f64_rate
// run:   ./f64_rate [waves per SIMD, 1..8, default 8]   (the running-mean kernel has two at 1080p)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
static int g_waves = 8;
#define ITERS 4096
template <int MODE>
__global__ void k(double *out, double a, double b)
{
    double acc[8];
    for (int i = 0; i < 8; i++) acc[i] = threadIdx.x + i;
    double x = a + threadIdx.x, y = b;
    uint32_t u = threadIdx.x;
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (MODE == 0) asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(x), "v"(y));
            if (MODE == 1) asm volatile("v_mul_f64 %0, %1, %0" : "+v"(acc[i]) : "v"(x));
            if (MODE == 2) asm volatile("v_add_f64 %0, %1, %0" : "+v"(acc[i]) : "v"(x));
            if (MODE == 3) asm volatile("v_cvt_f64_u32 %0, %1" : "=v"(acc[i]) : "v"(u));
            if (MODE == 4) { uint32_t r; asm volatile("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(acc[i])); u += r; }
            if (MODE == 5) { int r; asm volatile("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(acc[i])); u += r; }
            if (MODE == 6) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(acc[i]) : "v"(x), "v"(y));
            if (MODE == 7) asm volatile("v_perm_b32 %0, %1, %0, %2" : "+v"(u) : "v"(threadIdx.x), "v"(0x05040100u));
            if (MODE == 8) asm volatile("v_bfe_u32 %0, %0, 8, 8" : "+v"(u));
        }
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]), "+v"(u));
    }
    double s = u;
    for (int i = 0; i < 8; i++) s += acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
template <int MODE> void run(const char *name, double *d, int extra)
{
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    int blocks = 256 * g_waves, threads = 256;   // one wave per SIMD and block
    k<MODE><<<blocks, threads>>>(d, 3, 5);
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    k<MODE><<<blocks, threads>>>(d, 3, 5);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    double waveinstr = (double)blocks * threads / 64 * ITERS * 8 * (1 + extra);
    double per_simd = waveinstr / (256 * 4);
    printf("%-18s %.3f ms  -> %.2f cycles @2.4GHz per wave-instr per SIMD%s\n", name, ms, ms * 1e6 / per_simd * 2.4, extra ? " (incl. one v_add_u32 each)" : "");
}
int main(int argc, char **argv)
{
    if (argc > 1)
        g_waves = atoi(argv[1]);
    if (g_waves < 1 || g_waves > 8)
        g_waves = 8;
    printf("%d waves per SIMD\n", g_waves);
    double *d; (void)hipMalloc(&d, 256 * 8 * 256 * 8);
    run<0>("v_fma_f64", d, 0); run<1>("v_mul_f64", d, 0); run<2>("v_add_f64", d, 0); run<3>("v_cvt_f64_u32", d, 0);
    run<4>("v_cvt_u32_f64", d, 1); run<5>("v_cvt_i32_f64", d, 1);
    run<6>("v_fmac_f64", d, 0); run<7>("v_perm_b32", d, 0); run<8>("v_bfe_u32", d, 0);
    return 0;
}
