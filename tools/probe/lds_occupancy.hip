// How many workgroups of 192 threads the runtime's occupancy query places on a CU as their dynamic LDS grows (queries only, nothing is launched).
// Written for the 96-pixel form of conv3x3_split_kernel (profiles/r09_ab_c3_tile96.txt): the query divides the 160 KB byte for byte
// (4 workgroups up to 40 960 bytes, 3 up to 54 592, 2 up to 81 920) and shows no allocation block, although a gfx950 code object states its LDS in
// blocks of 1280 bytes - a launch rule that needs n workgroups per CU should count in those blocks.
//   hipcc --offload-arch=gfx950 -O2 tools/probe/lds_occupancy.hip -o tools/probe/lds_occupancy && tools/probe/lds_occupancy
#include <hip/hip_runtime.h>
#include <cstdio>

__global__ __launch_bounds__(192) void probe(float* out)
{
    extern __shared__ float s[];
    s[threadIdx.x] = (float)threadIdx.x;
    __syncthreads();
    if (out) out[threadIdx.x] = s[191 - threadIdx.x];
}

int main()
{
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(probe), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return 1;
    int prev = -1;
    for (int bytes = 40960; bytes <= 84 * 1024; bytes += 64) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, probe, 192, bytes) != hipSuccess) return 1;
        if (n != prev) printf("from %6d bytes (%.3f blocks of 1280): %d workgroups per CU\n", bytes, bytes / 1280.0, n);
        prev = n;
    }
    return 0;
}
