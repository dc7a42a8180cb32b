// act_norm_bench.hip — device times of the new streaming kernels of csrc/ops_act.hip next to the ones they sit beside:
//   k_glu<GEGLU> against k_swiglu at 512 x 14336 (split form), the fused k_norm (* w + b) against k_rms_norm (* w) at 512 x 4096.
// The question behind the first pair: what does GEGLU's 2-byte gather from a 128 KiB table cost against a streamed SwiGLU?
// Links the product's own objects (build_act_norm_bench.sh), so what is timed is what ships.  hipEvents around LAUNCHES back-to-back launches; the two
// kernels of a pair alternate within a round; every launch of a window works on another operand set, the sets together exceeding L2 and the 256 MiB MALL.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "kernels.h"

using namespace mi355x;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static constexpr int ROUNDS = 7, LAUNCHES = 200;

static tdesc desc2d(void * p, int64_t ne0, int64_t ne1) {
    tdesc d{};
    d.data = (char *) p;
    d.ne[0] = ne0; d.ne[1] = ne1; d.ne[2] = 1; d.ne[3] = 1;
    d.nb[0] = 4; d.nb[1] = 4 * ne0; d.nb[2] = d.nb[1] * ne1; d.nb[3] = d.nb[2];
    d.type = GGML_TYPE_F32;
    return d;
}

// per-launch microseconds of `fn(set)`: median, min and max over the rounds
struct timing { double med, lo, hi; };
static bool time_pair(hipStream_t s, int sets, const std::function<void(int)> & fa, const std::function<void(int)> & fb, timing & ta, timing & tb) {
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return false;
    std::vector<double> va, vb;
    for (int r = -1; r < ROUNDS; ++r) {  // (round -1: warm-up of both, not recorded)
        for (int which = 0; which < 2; ++which) {
            const auto & f = which ? fb : fa;
            (void) hipEventRecord(e0, s);
            for (int i = 0; i < LAUNCHES; ++i) f(i % sets);
            (void) hipEventRecord(e1, s);
            if (hipEventSynchronize(e1) != hipSuccess) return false;
            float ms = 0.f;
            (void) hipEventElapsedTime(&ms, e0, e1);
            if (r >= 0) (which ? vb : va).push_back(1000.0 * ms / LAUNCHES);
        }
    }
    auto stat = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return timing{v[v.size() / 2], v.front(), v.back()}; };
    ta = stat(va);
    tb = stat(vb);
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    return hipGetLastError() == hipSuccess;
}

int main() {
    hipStream_t s;
    CK(hipStreamCreate(&s));
    // the GELU table as the backend builds it (graph.cpp: act_tables_host); T_quick is not read here
    std::vector<uint16_t> tab(2 * 65536, 0);
    for (uint32_t i = 0; i < 65536; ++i) {
        const uint16_t u = (uint16_t) i;
        _Float16 hh;
        memcpy(&hh, &u, 2);
        const volatile float hv = (float) hh;
        const float x = hv;
        const _Float16 r = (_Float16) (0.5f * x * (1.0f + tanhf(0.79788456080286535588f * x * (1.0f + 0.044715f * x * x))));
        memcpy(&tab[i], &r, 2);
    }
    uint16_t * d_tab = nullptr;
    CK(hipMalloc((void **) &d_tab, tab.size() * 2));
    CK(hipMemcpy(d_tab, tab.data(), tab.size() * 2, hipMemcpyHostToDevice));

    std::mt19937 rng(1234);
    std::normal_distribution<float> nd(0.f, 2.f);  // FFN pre-activations: a few units wide, well inside the table's +-10
    std::vector<float> host((size_t) 512 * 14336);  // one draw, copied into every operand buffer
    for (auto & v : host) v = nd(rng);
    auto fill = [&](float * dev, size_t n) { return hipMemcpy(dev, host.data(), n * 4, hipMemcpyHostToDevice); };
    const size_t spill = (size_t) 600 << 20;  // operand sets together: above the MALL

    {   // GLU, split form: 512 rows x 14336
        const int64_t rows = 512, nc = 14336;
        const size_t n = (size_t) rows * nc, set_bytes = 3 * n * 4;
        const int sets = (int) ((spill + set_bytes - 1) / set_bytes);
        std::vector<float *> a(sets), b(sets), d(sets);
        for (int k = 0; k < sets; ++k) {
            CK(hipMalloc((void **) &a[k], n * 4)); CK(hipMalloc((void **) &b[k], n * 4)); CK(hipMalloc((void **) &d[k], n * 4));
            CK(fill(a[k], n)); CK(fill(b[k], n));
        }
        timing tg, ts;
        const bool ok = time_pair(s, sets,
            [&](int k) { const tdesc bd = desc2d(b[k], nc, rows); launch_glu(s, GGML_GLU_OP_GEGLU, desc2d(a[k], nc, rows), &bd, desc2d(d[k], nc, rows), 0, d_tab); },
            [&](int k) { const tdesc bd = desc2d(b[k], nc, rows); launch_swiglu(s, desc2d(a[k], nc, rows), &bd, desc2d(d[k], nc, rows), 0); }, tg, ts);
        if (!ok) { fprintf(stderr, "GLU timing failed\n"); return 1; }
        const double gb = 3.0 * n * 4 / 1e9;
        printf("glu 512 x 14336 split, %d operand sets, %d rounds x %d launches, us per launch median [min .. max]:\n", sets, ROUNDS, LAUNCHES);
        printf("  k_glu<GEGLU>  %8.2f [%8.2f .. %8.2f]   %7.0f GB/s\n", tg.med, tg.lo, tg.hi, gb / (tg.med * 1e-6));
        printf("  k_swiglu      %8.2f [%8.2f .. %8.2f]   %7.0f GB/s\n", ts.med, ts.lo, ts.hi, gb / (ts.med * 1e-6));
        printf("  GEGLU / SwiGLU = %.3f\n", tg.med / ts.med);
        for (int k = 0; k < sets; ++k) { (void) hipFree(a[k]); (void) hipFree(b[k]); (void) hipFree(d[k]); }
    }
    {   // NORM * w + b against RMS_NORM * w: 512 rows x 4096
        const int64_t rows = 512, ne0 = 4096;
        const size_t n = (size_t) rows * ne0, set_bytes = 2 * n * 4;
        const int sets = (int) ((spill + set_bytes - 1) / set_bytes);
        std::vector<float *> x(sets), y(sets);
        float * w = nullptr, * b = nullptr;
        CK(hipMalloc((void **) &w, ne0 * 4)); CK(hipMalloc((void **) &b, ne0 * 4));
        CK(fill(w, ne0)); CK(fill(b, ne0));
        for (int k = 0; k < sets; ++k) {
            CK(hipMalloc((void **) &x[k], n * 4)); CK(hipMalloc((void **) &y[k], n * 4));
            CK(fill(x[k], n));
        }
        timing tn, tr;
        const tdesc wd = desc2d(w, ne0, 1);
        const bool ok = time_pair(s, sets,
            [&](int k) { launch_norm(s, desc2d(x[k], ne0, rows), desc2d(y[k], ne0, rows), 1e-5f, w, b); },
            [&](int k) { launch_rms_norm(s, desc2d(x[k], ne0, rows), desc2d(y[k], ne0, rows), 1e-5f, &wd); }, tn, tr);
        if (!ok) { fprintf(stderr, "NORM timing failed\n"); return 1; }
        const double gb = 2.0 * n * 4 / 1e9;
        printf("norm 512 x 4096, %d operand sets, %d rounds x %d launches, us per launch median [min .. max]:\n", sets, ROUNDS, LAUNCHES);
        printf("  k_norm * w + b   %8.2f [%8.2f .. %8.2f]   %7.0f GB/s\n", tn.med, tn.lo, tn.hi, gb / (tn.med * 1e-6));
        printf("  k_rms_norm * w   %8.2f [%8.2f .. %8.2f]   %7.0f GB/s\n", tr.med, tr.lo, tr.hi, gb / (tr.med * 1e-6));
        printf("  NORM / RMS_NORM = %.3f\n", tn.med / tr.med);
    }
    return 0;
}
