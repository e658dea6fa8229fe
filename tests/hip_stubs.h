// Stubs of the HIP runtime for the host-only dispatch recorders (tests/dispatch_recorder.cpp, tests/row_recorder.cpp): the dozen
// runtime symbols a kernel object needs, hipLaunchKernel among them, which appends ` | <mangled kernel> <grid> <block> <dynamic LDS>`
// (and the scalar int arguments named in g_int_args) to the record of the call in flight instead of launching.  Include once per program.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

struct dim3 { unsigned x, y, z; };
typedef int hipError_t;
typedef struct ihipStream_t *hipStream_t;

namespace {
struct Kernel { const void *host; const char *name; };
Kernel g_kernels[1024];                                   // filled by the objects' static constructors: plain storage, no constructor of its own
int g_n_kernels = 0;
dim3 g_grid, g_block;
size_t g_lds;
std::string g_line;                                       // the record of the call in flight

const char *kernel_name(const void *host) {
    for (int i = 0; i < g_n_kernels; ++i)
        if (g_kernels[i].host == host) return g_kernels[i].name;
    return "?";
}
// scalar int arguments to print behind a launch: `count` of them from argument `first`, for kernels whose name contains `kernel`
struct IntArgs { const char *kernel; int first, count; };
const IntArgs *g_int_args = nullptr;                        // set by the program that wants scalar arguments printed
int g_n_int_args = 0;
}  // namespace

extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *handle; return &handle; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *name, unsigned, void *, void *, void *, void *, int *) {
    if (g_n_kernels < 1024) g_kernels[g_n_kernels++] = {host, name};
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
unsigned __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t) {
    g_grid = grid, g_block = block, g_lds = lds;
    return 0;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *stream) {
    *grid = g_grid, *block = g_block, *lds = g_lds, *stream = nullptr;
    return 0;
}
hipError_t hipLaunchKernel(const void *host, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t) {
    const char *name = kernel_name(host);
    char buf[96];
    snprintf(buf, sizeof buf, " %u,%u,%u %u %zu", grid.x, grid.y, grid.z, block.x, lds);
    g_line += " | ";
    g_line += name;
    g_line += buf;
    for (int a = 0; a < g_n_int_args; ++a) {
        const IntArgs &ia = g_int_args[a];
        if (strstr(name, ia.kernel))
            for (int i = 0; i < ia.count; ++i) {
                snprintf(buf, sizeof buf, "%c%d", i ? ',' : ' ', *(const int *)args[ia.first + i]);
                g_line += buf;
            }
    }
    return 0;
}
hipError_t hipGetLastError() { return 0; }
hipError_t hipFuncSetAttribute(const void *, int, int) { return 0; }
hipError_t hipGetDevice(int *dev) { *dev = 0; return 0; }
hipError_t hipDeviceGetAttribute(int *value, int, int) { *value = 256; return 0; }
}

