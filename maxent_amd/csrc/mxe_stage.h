// mxe_stage.h -- host side of the single-launch entry points of maxent_hip.hip ("How an entry point stages
// its call"): the checks they share, the layout of a block of arrays, and Stage, which owns what a call holds on the
// device.  Included by one translation unit, after mxe_ctx, stream_wait and the MXE_ERR_* codes are defined.
// With MXE_STAGE_PURE defined only the part that needs no HIP is compiled (tools/stage_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace {

// a NaN or an Inf anywhere: x - x is then NaN (eight independent chains)
inline bool all_finite(const double* x, size_t nel)
{
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t i = 0;
    for (; i + 8 <= nel; i += 8)
        for (int q = 0; q < 8; ++q) acc[q] += x[i + q] - x[i + q];
    for (; i < nel; ++i) acc[0] += x[i] - x[i];
    for (int q = 0; q < 8; ++q) if (acc[q] != 0.0) return false;
    return true;
}

// group g holds the rows [off[g], off[g + 1]): off[0] == 0 and no offset below the one before it; longest: the longest group
inline bool group_offsets_ok(const int32_t* off, int n_groups, int* longest = nullptr)
{
    if (off[0] != 0) return false;
    int len = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (off[g + 1] < off[g]) return false;
        if (off[g + 1] - off[g] > len) len = off[g + 1] - off[g];
    }
    if (longest) *longest = len;
    return true;
}

// The rows of the last launch a call reads when no H is handed in: out[r] = problem_index[r] (r where there is no index),
// each below n_last.
inline bool launch_rows(const int32_t* problem_index, size_t rows, size_t n_last, int* out)
{
    for (size_t r = 0; r < rows; ++r) {
        const int row = problem_index ? problem_index[r] : (int)r;
        if (row < 0 || (size_t)row >= n_last) return false;
        out[r] = row;
    }
    return true;
}

// Arrays laid back to back in one block: ``off = block.add(count)`` per array, in the order they lie; total: its size.
// The call site is the one description of a layout.
struct Block {
    size_t total = 0;
    size_t add(size_t count) { const size_t off = total; total += count; return off; }
};

} // namespace

#ifndef MXE_STAGE_PURE
#include <cstdio>
#include <string>
#include <vector>

// returns MXE_ERR_HIP from the entry at the first HIP call that fails (st: the Stage of the call)
#define STGCHK(st, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return (st).fail(#call, e__); } while (0)

namespace {

// What a call holds on the device, released on every path.  open(device): a context-free entry -- picks the device and
// works on a non-blocking stream of its own; open(ctx): works on the stream of the context.  A null host pointer or a
// count of zero makes upload and fetch a no-op: an optional array is handed over as it came.
struct Stage {
    mxe_ctx* ctx = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool timed = false;
    std::vector<void*> bufs;

    Stage() = default;
    Stage(const Stage&) = delete;                // (it frees what it owns: never passed by value)
    Stage& operator=(const Stage&) = delete;
    ~Stage() {
        for (void* b : bufs) hipFree(b);
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        if (stream && !ctx) hipStreamDestroy(stream);
    }
    // a failed HIP call: to the context where there is one, to stderr where there is none
    int fail(const char* what, hipError_t e) {
        if (ctx) ctx->hip_err = std::string(what) + ": " + hipGetErrorString(e);
        else fprintf(stderr, "[mxe] %s: %s\n", what, hipGetErrorString(e));
        return MXE_ERR_HIP;
    }
    int open(int device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return MXE_ERR_NODEVICE;
        if (device < 0 || device >= ndev) return MXE_ERR_ARG;
        STGCHK(*this, hipSetDevice(device));
        STGCHK(*this, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return MXE_OK;
    }
    int open(mxe_ctx* c) {
        ctx = c; stream = c->stream;
        STGCHK(*this, hipSetDevice(c->device));
        return MXE_OK;
    }
    template <typename T> hipError_t alloc(T** p, size_t count) {
        hipError_t e = hipMalloc((void**)p, (count > 0 ? count : 1) * sizeof(T));
        if (e == hipSuccess) bufs.push_back((void*)*p);
        return e;
    }
    // into an owned array or into a place of a context's block
    template <typename T> hipError_t upload(T* dst, const T* src, size_t count) {
        if (!src || !count) return hipSuccess;
        return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
    }
    template <typename T> hipError_t fetch(T* dst, const T* src, size_t count) {
        if (!dst || !count) return hipSuccess;
        return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, stream);
    }
    // the time of what is queued between time_begin and time_end, when wanted: finish hands it out
    hipError_t time_begin(bool wanted) {
        if (!wanted) return hipSuccess;
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess) e = hipEventRecord(e0, stream);
        timed = e == hipSuccess;
        return e;
    }
    hipError_t time_end() { return timed ? hipEventRecord(e1, stream) : hipSuccess; }
    // waits for the stream (a context's: by polling, stream_wait); after it the fetched arrays are the caller's
    hipError_t finish(float* out_ms) {
        hipError_t e = ctx ? stream_wait(stream) : hipStreamSynchronize(stream);
        if (e == hipSuccess && timed) e = hipEventElapsedTime(out_ms, e0, e1);
        return e;
    }
};

// kernel k with lds bytes of dynamic LDS: raises the limit of the kernel, launches it, reports the launch
template <typename... KArgs, typename... Args>
hipError_t launch_lds(void (*k)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args)
{
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, grid, block, lds, s, args...);
    return hipGetLastError();
}

} // namespace
#endif
