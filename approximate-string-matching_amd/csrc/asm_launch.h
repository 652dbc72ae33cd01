// The one kernel launch of this library.  Every host launcher goes through launch_on (or through launch / launch_lds, its forms
// behind the handle in asm_capi.hip), which returns the launch's error: the caller checks it where the call is made, so a kernel
// that reads another kernel's output is never enqueued behind a launch that failed.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

/* `grid` workgroups of `block` threads with `lds` bytes of dynamic LDS on `stream`.  More than 64 KiB of dynamic LDS has to be asked
 * for, per kernel: done here, so a launcher only states the size. */
template <class... P, class... A>
static inline hipError_t launch_on(hipStream_t stream, void (*kernel)(P...), unsigned grid, unsigned block, size_t lds, A&&... args) {
    if (lds > 64 * 1024)
        if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, std::forward<A>(args)...);
    return hipGetLastError();
}
