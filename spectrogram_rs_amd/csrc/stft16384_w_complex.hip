// stft16384_w_complex.hip -- the complex-row instantiations of the 16384-point kernel (sgx_stft_batch_complex): the device code of
// stft16384_w_kernels.hpp with SGX_W16K_C64, in a namespace of its own, and their launcher.
#define SGX_W16K_C64 1
#define SGX_W16K_NS w16kc
#include "stft16384_w_kernels.hpp"

#include <cstring>

namespace sgx {

// params: the w16k::Params that launch_w16384 (stft16384_w.hip) filled (the same definition, compiled into w16kc here)
hipError_t launch_w16384_complex(const void *params, size_t params_size, bool mono, bool slide, bool direct, dim3 grid, hipStream_t stream)
{
    using namespace w16kc;
    Params p;
    if (params_size != sizeof p) return hipErrorInvalidValue;
    std::memcpy(&p, params, sizeof p);
    const void *k = mono             ? reinterpret_cast<const void *>(stft16384_w_kernel<true>)
                    : slide && direct ? reinterpret_cast<const void *>(stft16384_w_kernel<false, true, true>)
                    : slide           ? reinterpret_cast<const void *>(stft16384_w_kernel<false, false, true>)
                    : direct          ? reinterpret_cast<const void *>(stft16384_w_kernel<false, true>)
                                      : reinterpret_cast<const void *>(stft16384_w_kernel<false>);
    // per launch: the attribute is per device, and a process may hold contexts on several
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return e;
    const dim3 block(512);
    if (mono) hipLaunchKernelGGL((stft16384_w_kernel<true>), grid, block, kLdsBytes, stream, p);
    else if (slide && direct) hipLaunchKernelGGL((stft16384_w_kernel<false, true, true>), grid, block, kLdsBytes, stream, p);
    else if (slide) hipLaunchKernelGGL((stft16384_w_kernel<false, false, true>), grid, block, kLdsBytes, stream, p);
    else if (direct) hipLaunchKernelGGL((stft16384_w_kernel<false, true>), grid, block, kLdsBytes, stream, p);
    else hipLaunchKernelGGL((stft16384_w_kernel<false>), grid, block, kLdsBytes, stream, p);
    return hipGetLastError();
}

}  // namespace sgx
