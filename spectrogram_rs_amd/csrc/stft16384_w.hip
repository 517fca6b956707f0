// stft16384_w.hip -- the magnitude rows of the tuned 16384-point STFT (W = 8192; the design: stft16384_w_kernels.hpp) and the host code of
// both its forms: tables, job split and launches.
#define SGX_W16K_C64 0
#define SGX_W16K_NS w16k
#include "stft16384_w_kernels.hpp"

namespace sgx {

#if SGX_STAMPS
extern "C" __attribute__((visibility("default"))) int sgx_debug_phase_cycles16w(unsigned long long *h_out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(h_out, HIP_SYMBOL(w16k::g_phase_cycles16w), sizeof(unsigned long long) * 24);
    if (e == hipSuccess && reset) {
        unsigned long long zero[24] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(w16k::g_phase_cycles16w), zero, sizeof(zero));
    }
    return e == hipSuccess ? 0 : -1;
}
#endif

bool w16384_supported(const sgx_ctx *c)
{
    // (l, r) pairs are moved as 8-byte words: the stream must be mono or have an even channel count
    return c->W == w16k::kW && (c->C == 1 || (c->C & 1) == 0) && c->lds_optin >= w16k::kLdsBytes;
}

void TablesDelete::operator()(w16k::TablesW *t) const { delete t; }

hipError_t w16384_init(sgx_ctx *c)
{
    using namespace w16k;
    TablesPtr<TablesW> t(new TablesW());
    std::vector<float2> T1(32 * 512), tw2(512);
    std::vector<float> win16((size_t)kW);
    for (int q = 0; q < 32; ++q)
        for (int cc = 0; cc < 512; ++cc) T1[q * 512 + cc] = unit_root2((unsigned long long)q * cc, kP);
    for (int c0 = 0; c0 < 16; ++c0)
        for (int q2 = 0; q2 < 32; ++q2) tw2[c0 * 32 + q2] = unit_root2((unsigned long long)q2 * c0, 512);
    // the scale (hypot / 2) * (2 / W) = 1 / W is a power of two and commutes with every rounding
    for (int a = 0; a < 16; ++a)
        for (int cc = 0; cc < 512; ++cc) win16[((size_t)(a >> 2) * 512 + cc) * 4 + (a & 3)] = c->tab.window[cc + 512 * a] * (1.0f / (float)kW);
    hipError_t e = t->d_T1.upload(T1);
    if (e == hipSuccess) e = t->d_tw2.upload(tw2);
    if (e == hipSuccess) e = t->d_win16.upload(win16);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(stft16384_w_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(stft16384_w_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(stft16384_w_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(stft16384_w_kernel<false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(stft16384_w_kernel<false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e == hipSuccess) c->w16k = std::move(t);
    return e;
}

// stft16384_w_complex.hip: the complex-row kernels, launched on this file's parameter block (the same struct there)
hipError_t launch_w16384_complex(const void *params, size_t params_size, bool mono, bool slide, bool direct, dim3 grid, hipStream_t stream);

hipError_t launch_w16384(const sgx_ctx *c, const StftCall &call)
{
    using namespace w16k;
    if (call.kind != Out::kMags && call.kind != Out::kComplex) return hipErrorInvalidValue;
    const bool complex_rows = call.kind == Out::kComplex;
    const float *d_pcm = call.pcm;
    float *d_mags = static_cast<float *>(call.out);
    const uint32_t channels = call.channels, pairs = call.pairs;
    const size_t first_frame = call.first, n_frames = call.n, total_frames = call.total;
    if (n_frames == 0) return hipSuccess;
    TablesW *t = c->w16k.get();   // (not const: the plane below is regrown)
    Params p{};
    p.T1 = t->d_T1.get();
    p.tw2 = t->d_tw2.get();
    p.win16 = t->d_win16.get();
    p.mags = d_mags;
    p.first_frame = first_frame;
    p.n_frames = n_frames;
    p.total_frames = total_frames;
    p.H = c->H;
    p.pairs = pairs;
    // (a hop whose frame pairs do not fit a descriptor takes the route of unpaired frames)
    const bool mono = paired_mono(c, channels) && descriptor_pairs_fit(c->H, kW);
    // a mono stream whose frames are not paired (the default): every frame the (s, s) transform of the reference
    // (audio_input_list_model.rs:67-69) -- the sample range duplicated into one (s, s) plane, then the two-channel kernel
    const bool dup = channels == 1 && !mono;
    p.pair_base = mono ? first_frame / 2 : 0;
    p.n_jobs = mono ? (first_frame + n_frames + 1) / 2 - first_frame / 2 : (unsigned long long)n_frames * pairs;
    const bool direct = channels > 2;     // every pair read where it lies: no workspace, no second kernel
    // lane offsets are 32-bit: 4 C (511 + 512 * 15) + 8 bytes must stay below the descriptor's 2^31 - 1 records (sgx_create caps C)
    if (direct && (unsigned long long)channels * 32764ull + 8ull >= 0x7fffffffull) return hipErrorInvalidValue;
    if (dup) {
        const size_t first_sample = first_frame * (size_t)c->H;
        const size_t n_samp = (n_frames - 1) * (size_t)c->H + kW;
        const size_t plane = (2 * n_samp + 63) & ~(size_t)63;  // floats
        hipError_t e = t->d_planes.grow(c->stream, plane);   // (a previous launch may still read the old plane)
        if (e != hipSuccess) return e;
        const unsigned blocks = (unsigned)std::min<size_t>((n_samp + 255) / 256, (size_t)c->n_cu * 16);
        hipLaunchKernelGGL(w16k::duplicate_mono_kernel, dim3(blocks), dim3(256), 0, c->stream, d_pcm, t->d_planes.get(), first_sample, n_samp);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        p.pcm = t->d_planes.get();
        p.plane_floats = plane;
        p.sample_base = (long long)first_sample;
    } else {
        p.pcm = d_pcm;
        p.plane_floats = 0;
        p.sample_base = 0;
        p.stride_floats = channels;
    }
    // persistent workgroups, one per CU (132 KB of LDS); jobs are dealt round-robin in output-row order
    unsigned long long blocks = (unsigned long long)c->n_cu;
    if (blocks > p.n_jobs) blocks = p.n_jobs;
    p.xcds = (blocks % kXcdHint == 0 && p.n_jobs >= kXcdHint * blocks) ? kXcdHint : 1u;   // (short launches: plain round-robin keeps every workgroup busy)
    const unsigned long long group = mono ? 1 : pairs;                   // a hop position's pairs stay together
    p.jobs_per_xcd = ((p.n_jobs + p.xcds - 1) / p.xcds + group - 1) / group * group;
    // H = 512 (config 4's hop): the sliding window -- runs of hop positions, one pair per workgroup
    const bool slide = !mono && c->H == 512 && pairs <= (unsigned long long)c->n_cu;
    if (slide) {
        unsigned long long runs = (unsigned long long)c->n_cu / pairs;
        if (runs > n_frames) runs = n_frames;
        p.run_len = (n_frames + runs - 1) / runs;
        runs = (n_frames + p.run_len - 1) / p.run_len;
        blocks = runs * pairs;
        p.xcds = blocks % kXcdHint == 0 ? kXcdHint : 1u;
    }
    const dim3 grid((unsigned)blocks), block(512);
    if (complex_rows) return launch_w16384_complex(&p, sizeof p, mono, slide, direct, grid, c->stream);   // stft16384_w_complex.hip
    if (mono) hipLaunchKernelGGL((stft16384_w_kernel<true>), grid, block, kLdsBytes, c->stream, p);
    else if (slide && direct) hipLaunchKernelGGL((stft16384_w_kernel<false, true, true>), grid, block, kLdsBytes, c->stream, p);
    else if (slide) hipLaunchKernelGGL((stft16384_w_kernel<false, false, true>), grid, block, kLdsBytes, c->stream, p);
    else if (direct) hipLaunchKernelGGL((stft16384_w_kernel<false, true>), grid, block, kLdsBytes, c->stream, p);
    else hipLaunchKernelGGL((stft16384_w_kernel<false>), grid, block, kLdsBytes, c->stream, p);
    return hipGetLastError();
}

}  // namespace sgx
