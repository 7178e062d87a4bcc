// wavechain_team_reset.hip -- the one reset kernel in front of the team launches of the three wave-chain kernels (lenv_host::team_reset, lenv_host.h)
#include "lenv_host.h"

namespace lenv {
// the team barrier counters start at 0: a kernel rather than a memset node (see the status word in the fused kernels)
__global__ void wc_team_reset_kernel(float *arena, int64_t arena_stride, int64_t a_bar, int64_t chains)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < chains) { unsigned *b = reinterpret_cast<unsigned *>(arena + c * arena_stride + a_bar); b[0] = 0u; b[8] = 0u; }
#ifdef LENV_DIAG_TEAM_TIMES
    if (c == 0) *reinterpret_cast<unsigned long long *>(arena + a_bar + 10) = __builtin_amdgcn_s_memrealtime();
#endif
}
}

void lenv_host::team_reset(float *arena, int64_t arena_stride, int64_t a_bar, int64_t chains, hipStream_t stream)
{
    hipLaunchKernelGGL(lenv::wc_team_reset_kernel, dim3((unsigned)((chains + 255) / 256)), dim3(256), 0, stream, arena, arena_stride, a_bar, chains);
}
