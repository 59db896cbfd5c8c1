/* Layer 3: the residual (transform unit) path on the GPU (include/x265amd.h, `x265amd_tu_*`).
 *
 * Device restatement of Quant::transformNxN without RDOQ (reference: source/common/quant.cpp:397-480), its sign-bit
 * hiding (quant.cpp:247-395, scanPosLast dct.cpp:757-788), Quant::invtransformNxN (quant.cpp:543-605) and the per-TU
 * measurement of Search::estimateResidualQT (source/encoder/search.cpp:3276-3330): one 64-lane wavefront per TU, all
 * intermediate blocks in LDS.  Sign-bit hiding treats every 4x4 coefficient group independently, so it runs one lane
 * per group (64 groups in a 32x32 TU).  Integer arithmetic, bit-exact with the reference.
 */
#include "x265amd_dev.h"
#include "x265amd_host.h"
#include "tu_dev.h"
#include "intra_pu_dev.h"
#include "xa_queue.h"
#include <math.h>
#include <string.h>

template<bool RDOQ>
__global__ __launch_bounds__(64 * (RDOQ ? TU_RDOQ_WAVES : TU_WAVES)) void k_tu_chain(const x265amd_tu_job* jobs, const x265amd_tu_rdoq* rq, int n, x265amd_tu_result* out)
{
    extern __shared__ __attribute__((aligned(16))) char tu_smem[];
    constexpr int WAVES = RDOQ ? TU_RDOQ_WAVES : TU_WAVES;
    const int lane = xa_lane(), wv = threadIdx.x >> 6;
    const int ji = blockIdx.x * WAVES + wv;
    if (ji >= n) return;
    TuLds& s = reinterpret_cast<TuLds*>(tu_smem)[wv];
    wave_tu_chain_job<RDOQ>(jobs, rq, ji, out, s, RDOQ ? tu_smem + WAVES * sizeof(TuLds) + wv * sizeof(RdoqLds) : nullptr, lane);
}

template<bool RDOQ>
__global__ __launch_bounds__(64 * (RDOQ ? TU_RDOQ_WAVES : TU_WAVES)) void k_intra_tu_chain(const x265amd_intra_tu_job* jobs, const x265amd_tu_rdoq* rq, int n,
                                                                                          x265amd_tu_result* out)
{
    extern __shared__ __attribute__((aligned(16))) char tu_smem[];
    constexpr int WAVES = RDOQ ? TU_RDOQ_WAVES : TU_WAVES;
    const int lane = xa_lane(), wv = threadIdx.x >> 6;
    const int ji = blockIdx.x * WAVES + wv;
    if (ji >= n) return;
    TuLds& s = reinterpret_cast<TuLds*>(tu_smem)[wv];
    char* extra = tu_smem + WAVES * sizeof(TuLds);
    IntraTuLds& ip = reinterpret_cast<IntraTuLds*>(extra)[wv];
    wave_intra_tu_chain_job<RDOQ>(jobs, rq, ji, out, s, ip, RDOQ ? extra + WAVES * sizeof(IntraTuLds) + wv * sizeof(RdoqLds) : nullptr, lane);
}

/* the two Quant entry points on their own (parity surface): op 0 forward (a = residual in, coeff out, numSig -> out),
 * op 1 inverse (coeff in, residual out) */
struct TuSoloJob { uint64_t in, outp, numSigOut; int32_t stride, op, log2N, ttype, intra, dirMode, sliceType, qpScaled, signHide, numSig;
                   uint64_t fenc, est; int64_t lambda2; int32_t fencStride, lambda, psyRdoqScale, rdoqLevel, tuDepth; };

__global__ __launch_bounds__(64) void k_tu_solo(TuSoloJob j)
{
    extern __shared__ __attribute__((aligned(16))) char tu_smem[];
    TuLds& s = *reinterpret_cast<TuLds*>(tu_smem);
    const int lane = xa_lane(), N = 1 << j.log2N, numCoeff = N * N;
    if (j.op == 0)
    {
        const int16_t* resi = reinterpret_cast<const int16_t*>(j.in);
        for (int i = lane; i < numCoeff; i += XA_WAVE) s.a[i] = resi[(i >> j.log2N) * j.stride + (i & (N - 1))];
        xa_wave_sync();
        uint32_t ns;
        if (j.rdoqLevel)
        {
            RdoqLds& r = *reinterpret_cast<RdoqLds*>(tu_smem + sizeof(TuLds));
            RdoqParams P = { reinterpret_cast<const int*>(j.est), j.lambda2, j.lambda, j.psyRdoqScale, j.rdoqLevel, j.tuDepth };
            ns = wave_tu_forward_rdoq(s, r, P, reinterpret_cast<const pixel*>(j.fenc), j.fencStride, j.log2N, j.ttype, j.intra, j.dirMode, j.qpScaled, j.signHide, 0, lane);
        }
        else ns = wave_tu_forward(s, j.log2N, j.ttype, j.intra, j.dirMode, j.sliceType, j.qpScaled, j.signHide, 0, lane);
        int16_t* coeff = reinterpret_cast<int16_t*>(j.outp);
        for (int i = lane; i < numCoeff; i += XA_WAVE) coeff[i] = s.q[i];
        if (lane == 0) *reinterpret_cast<uint64_t*>(j.numSigOut) = ns;
    }
    else
    {
        const int16_t* coeff = reinterpret_cast<const int16_t*>(j.in);
        for (int i = lane; i < numCoeff; i += XA_WAVE) s.q[i] = coeff[i];
        xa_wave_sync();
        wave_tu_inverse(s, j.log2N, j.ttype, j.intra, j.qpScaled, (uint32_t)j.numSig, lane);
        int16_t* resi = reinterpret_cast<int16_t*>(j.outp);
        for (int i = lane; i < numCoeff; i += XA_WAVE) resi[(i >> j.log2N) * j.stride + (i & (N - 1))] = s.a[i];
    }
}

#define INTRA_PU_WAVES 8
constexpr size_t kIntraPuLds = (sizeof(IntraScanLds) > INTRA_PU_WAVES * (sizeof(TuLds) + sizeof(IntraTuLds)) ? sizeof(IntraScanLds) : INTRA_PU_WAVES * (sizeof(TuLds) + sizeof(IntraTuLds))) + sizeof(Nxn4Lds);      /* + the chroma working set of an 8x8 2Nx2N CU behind the luma chains' (block_intra_nxn: chromaAhead) */
__global__ __launch_bounds__(64 * INTRA_PU_WAVES) void k_intra_pu(const x265amd_intra_pu_job* job, x265amd_intra_pu_out* out, x265amd_tu_result* res)
{
    extern __shared__ __attribute__((aligned(16))) char tu_smem[];
    block_intra_pu(job, out, res, tu_smem, threadIdx.x, 64 * INTRA_PU_WAVES);
}

__global__ __launch_bounds__(64 * INTRA_PU_WAVES) void k_intra_nxn(const x265amd_intra_nxn_job* job, x265amd_intra_nxn_out* out, int n, long strideBytes)
{
    extern __shared__ __attribute__((aligned(16))) char tu_smem[];
    for (int i = 0; i < n; i++)
        block_intra_nxn(reinterpret_cast<const x265amd_intra_nxn_job*>(reinterpret_cast<const char*>(job) + (size_t)i * strideBytes), out, tu_smem, threadIdx.x, 64 * INTRA_PU_WAVES, (int)kIntraPuLds);
}

/* =========================================================================================================
 * host side
 * ======================================================================================================= */
static int tu_configure()
{
    static thread_local bool done = false;
    if (!done)
    {
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_tu_chain<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(TU_WAVES * sizeof(TuLds))));
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_tu_chain<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(TU_RDOQ_WAVES * (sizeof(TuLds) + sizeof(RdoqLds)))));
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_tu_solo, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(TuLds) + sizeof(RdoqLds))));
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_intra_tu_chain<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(TU_WAVES * (sizeof(TuLds) + sizeof(IntraTuLds)))));
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_intra_tu_chain<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(TU_RDOQ_WAVES * (sizeof(TuLds) + sizeof(IntraTuLds) + sizeof(RdoqLds)))));
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_intra_pu, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIntraPuLds));
        XA_HIP_CHECK(hipFuncSetAttribute((const void*)k_intra_nxn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kIntraPuLds));
        done = true;
    }
    return X265AMD_OK;
}

extern "C" int x265amd_tu_chain(void* stream, const x265amd_tu_job* d_jobs, int n, x265amd_tu_result* d_out)
{
    if (n <= 0) return X265AMD_OK;
    if (!d_jobs || !d_out) return xa_fail(X265AMD_EINVAL, "x265amd_tu_chain: bad arguments");
    int rc = xa_is_queue(stream) ? X265AMD_OK : tu_configure();
    if (rc) return rc;
    const XaArgsJobs4 qa = { (uint64_t)(uintptr_t)d_jobs, 0, (uint64_t)(uintptr_t)d_out, 0, n };
    hipError_t e;
    XA_LAUNCH(e, stream, XA_OP_TU_CHAIN, n, qa, k_tu_chain<false>, dim3((n + TU_WAVES - 1) / TU_WAVES), dim3(64 * TU_WAVES), TU_WAVES * sizeof(TuLds), d_jobs,
                             (const x265amd_tu_rdoq*)nullptr, n, d_out);
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_tu_chain_rdoq(void* stream, const x265amd_tu_job* d_jobs, const x265amd_tu_rdoq* d_rdoq, int n, x265amd_tu_result* d_out)
{
    if (n <= 0) return X265AMD_OK;
    if (!d_jobs || !d_rdoq || !d_out) return xa_fail(X265AMD_EINVAL, "x265amd_tu_chain_rdoq: bad arguments");
    int rc = xa_is_queue(stream) ? X265AMD_OK : tu_configure();
    if (rc) return rc;
    const XaArgsJobs4 qa = { (uint64_t)(uintptr_t)d_jobs, (uint64_t)(uintptr_t)d_rdoq, (uint64_t)(uintptr_t)d_out, 0, n };
    hipError_t e;
    XA_LAUNCH(e, stream, XA_OP_TU_CHAIN_RDOQ, n, qa, k_tu_chain<true>, dim3((n + TU_RDOQ_WAVES - 1) / TU_RDOQ_WAVES), dim3(64 * TU_RDOQ_WAVES),
                             TU_RDOQ_WAVES * (sizeof(TuLds) + sizeof(RdoqLds)), d_jobs, d_rdoq, n, d_out);
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_intra_tu_chain(void* stream, const x265amd_intra_tu_job* d_jobs, const x265amd_tu_rdoq* d_rdoq, int n, x265amd_tu_result* d_out)
{
    if (n <= 0) return X265AMD_OK;
    if (!d_jobs || !d_out) return xa_fail(X265AMD_EINVAL, "x265amd_intra_tu_chain: bad arguments");
    int rc = xa_is_queue(stream) ? X265AMD_OK : tu_configure();
    if (rc) return rc;
    const XaArgsJobs4 qa = { (uint64_t)(uintptr_t)d_jobs, (uint64_t)(uintptr_t)d_rdoq, (uint64_t)(uintptr_t)d_out, 0, n };
    hipError_t e;
    if (d_rdoq)
        XA_LAUNCH(e, stream, XA_OP_INTRA_TU_CHAIN_RDOQ, n, qa, k_intra_tu_chain<true>, dim3((n + TU_RDOQ_WAVES - 1) / TU_RDOQ_WAVES), dim3(64 * TU_RDOQ_WAVES),
                      TU_RDOQ_WAVES * (sizeof(TuLds) + sizeof(IntraTuLds) + sizeof(RdoqLds)), d_jobs, d_rdoq, n, d_out);
    else
        XA_LAUNCH(e, stream, XA_OP_INTRA_TU_CHAIN, n, qa, k_intra_tu_chain<false>, dim3((n + TU_WAVES - 1) / TU_WAVES), dim3(64 * TU_WAVES),
                      TU_WAVES * (sizeof(TuLds) + sizeof(IntraTuLds)), d_jobs, (const x265amd_tu_rdoq*)nullptr, n, d_out);
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_intra_pu(void* stream, const x265amd_intra_pu_job* d_job, x265amd_intra_pu_out* d_out, x265amd_tu_result* d_res)
{
    if (!d_job || !d_out || !d_res) return xa_fail(X265AMD_EINVAL, "x265amd_intra_pu: bad arguments");
    int rc = xa_is_queue(stream) ? X265AMD_OK : tu_configure();
    if (rc) return rc;
    const XaArgsJobs4 qa = { (uint64_t)(uintptr_t)d_job, (uint64_t)(uintptr_t)d_out, (uint64_t)(uintptr_t)d_res, 0, 1 };
    hipError_t e;
    XA_LAUNCH(e, stream, XA_OP_INTRA_PU, 1, qa, k_intra_pu, dim3(1), dim3(64 * INTRA_PU_WAVES), kIntraPuLds, d_job, d_out, d_res);
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_intra_nxn(void* stream, const x265amd_intra_nxn_job* d_job, x265amd_intra_nxn_out* d_out)
{
    if (!d_job || !d_out) return xa_fail(X265AMD_EINVAL, "x265amd_intra_nxn: bad arguments");
    int rc = xa_is_queue(stream) ? X265AMD_OK : tu_configure();
    if (rc) return rc;
    const XaArgsJobs4 qa = { (uint64_t)(uintptr_t)d_job, (uint64_t)(uintptr_t)d_out, 0, 0, 1 };
    hipError_t e;
    XA_LAUNCH(e, stream, XA_OP_INTRA_NXN, 1, qa, k_intra_nxn, dim3(1), dim3(64 * INTRA_PU_WAVES), kIntraPuLds, d_job, d_out, 1, 0l);
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

extern "C" int x265amd_intra_nxn_list(void* stream, const x265amd_intra_nxn_job* d_jobs, int n, size_t stride_bytes, x265amd_intra_nxn_out* d_out)
{
    if (!d_jobs || !d_out || n < 1 || n > 64 || (stride_bytes & 7)) return xa_fail(X265AMD_EINVAL, "x265amd_intra_nxn_list: bad arguments");
    int rc = xa_is_queue(stream) ? X265AMD_OK : tu_configure();
    if (rc) return rc;
    const XaArgsJobs4 qa = { (uint64_t)(uintptr_t)d_jobs, (uint64_t)(uintptr_t)d_out, (uint64_t)stride_bytes, 0, n };
    hipError_t e;
    XA_LAUNCH(e, stream, XA_OP_INTRA_NXN, 1, qa, k_intra_nxn, dim3(1), dim3(64 * INTRA_PU_WAVES), kIntraPuLds, d_jobs, d_out, n, (long)stride_bytes);
    if (e != hipSuccess) return xa_fail(X265AMD_EHIP, hipGetErrorString(e));
    return X265AMD_OK;
}

/* QpParam::setQpParam (quant.h:50-60): the FIX8 lambdas RDOQ works with, from the tables' generating rules */
static double rd_lambda(int qp);
static double rd_lambda2(int qp);
extern "C" void x265amd_rdoq_lambda(int qpScaled, int64_t* lambda2, int32_t* lambda)
{
    const int qp = qpScaled - 6 * (X265AMD_DEPTH - 8);
    *lambda2 = (int64_t)(rd_lambda2(qp) * 256. + 0.5);
    *lambda = (int32_t)(rd_lambda(qp) * 256. + 0.5);
}

namespace {
struct Staging
{
    char* dev = nullptr;
    ~Staging() { if (dev) (void)hipFree(dev); }
    char* get() { if (!dev) XA_HIP_FATAL(hipMalloc((void**)&dev, 64 * 1024)); return dev; }
};
thread_local Staging g_stage;
}

static uint32_t transform_tu_host(const x265amd_pixel* fenc, intptr_t fencStride, const int16_t* resi, intptr_t resiStride, int16_t* coeff,
                                  int log2TrSize, int ttype, int bIntra, int dirMode, int sliceType, int qpScaled, int signHide,
                                  int tuDepth, int rdoqLevel, int psyRdoqScale, const int32_t* est)
{
    const int N = 1 << log2TrSize;
    if (tu_configure()) { fprintf(stderr, "x265amd: fatal: %s\n", x265amd_last_error()); abort(); }
    char* d = g_stage.get();
    int16_t* dResi = (int16_t*)d; int16_t* dCoeff = (int16_t*)(d + 4096); uint64_t* dNs = (uint64_t*)(d + 8192);
    x265amd_pixel* dFenc = (x265amd_pixel*)(d + 12288); int32_t* dEst = (int32_t*)(d + 16384);
    XA_HIP_FATAL(hipMemcpy2D(dResi, N * 2, resi, resiStride * 2, N * 2, N, hipMemcpyHostToDevice));
    TuSoloJob j = { (uint64_t)(uintptr_t)dResi, (uint64_t)(uintptr_t)dCoeff, (uint64_t)(uintptr_t)dNs, N, 0, log2TrSize, ttype, bIntra, dirMode, sliceType, qpScaled, signHide, 0,
                    0, 0, 0, 0, 0, 0, 0, 0 };
    if (rdoqLevel)
    {
        XA_HIP_FATAL(hipMemcpy2D(dFenc, N * sizeof(x265amd_pixel), fenc, fencStride * sizeof(x265amd_pixel), N * sizeof(x265amd_pixel), N, hipMemcpyHostToDevice));
        XA_HIP_FATAL(hipMemcpy(dEst, est, 184 * sizeof(int32_t), hipMemcpyHostToDevice));
        j.fenc = (uint64_t)(uintptr_t)dFenc; j.fencStride = N; j.est = (uint64_t)(uintptr_t)dEst;
        x265amd_rdoq_lambda(qpScaled, &j.lambda2, &j.lambda);
        j.psyRdoqScale = psyRdoqScale; j.rdoqLevel = rdoqLevel; j.tuDepth = tuDepth;
    }
    hipLaunchKernelGGL(k_tu_solo, dim3(1), dim3(64), sizeof(TuLds) + sizeof(RdoqLds), 0, j);
    XA_HIP_FATAL(hipGetLastError());
    uint64_t ns = 0;
    XA_HIP_FATAL(hipMemcpy(&ns, dNs, 8, hipMemcpyDeviceToHost));
    XA_HIP_FATAL(hipMemcpy(coeff, dCoeff, N * N * 2, hipMemcpyDeviceToHost));
    return (uint32_t)ns;
}

extern "C" uint32_t x265amd_transform_tu(const x265amd_pixel* fenc, intptr_t fencStride, const int16_t* resi, intptr_t resiStride, int16_t* coeff,
                                         int log2TrSize, int ttype, int bIntra, int dirMode, int sliceType, int qpScaled, int signHide)
{
    return transform_tu_host(fenc, fencStride, resi, resiStride, coeff, log2TrSize, ttype, bIntra, dirMode, sliceType, qpScaled, signHide, 0, 0, 0, nullptr);
}

extern "C" uint32_t x265amd_transform_tu_rdoq(const x265amd_pixel* fenc, intptr_t fencStride, const int16_t* resi, intptr_t resiStride, int16_t* coeff,
                                              int log2TrSize, int ttype, int bIntra, int dirMode, int sliceType, int qpScaled, int signHide,
                                              int tuDepth, int rdoqLevel, int psyRdoqScale, const int32_t* est)
{
    return transform_tu_host(fenc, fencStride, resi, resiStride, coeff, log2TrSize, ttype, bIntra, dirMode, sliceType, qpScaled, signHide,
                             tuDepth, rdoqLevel, psyRdoqScale, est);
}

extern "C" void x265amd_invtransform_tu(int16_t* resi, intptr_t resiStride, const int16_t* coeff, int log2TrSize, int ttype, int bIntra, int qpScaled, uint32_t numSig)
{
    const int N = 1 << log2TrSize;
    char* d = g_stage.get();
    int16_t* dResi = (int16_t*)d; int16_t* dCoeff = (int16_t*)(d + 4096);
    XA_HIP_FATAL(hipMemcpy(dCoeff, coeff, N * N * 2, hipMemcpyHostToDevice));
    TuSoloJob j = { (uint64_t)(uintptr_t)dCoeff, (uint64_t)(uintptr_t)dResi, 0, N, 1, log2TrSize, ttype, bIntra, 0, 1, qpScaled, 0, (int32_t)numSig,
                    0, 0, 0, 0, 0, 0, 0, 0 };
    hipLaunchKernelGGL(k_tu_solo, dim3(1), dim3(64), sizeof(TuLds), 0, j);
    XA_HIP_FATAL(hipGetLastError());
    XA_HIP_FATAL(hipMemcpy2D(resi, resiStride * 2, dResi, N * 2, N * 2, N, hipMemcpyDeviceToHost));
}

/* RDCost: rdcost.h:50-153.  x265_lambda_tab / x265_lambda2_tab (constants.cpp:34-150) are reproduced from their
 * generating rules (lambda: 2^(qp/6-2) rounded to 4 decimals, times 2^(depth-8); lambda2: 0.038*e^(0.234 qp) cut to 4
 * decimals, times 4^(depth-8)); all 70 entries of both are pinned against the reference by the parity tests. */
static double rd_lambda(int qp)
{
    double v = pow(2.0, (double)qp / 6.0 - 2.0) * (double)(1 << (X265AMD_DEPTH - 8));
    return floor(v * 10000.0 + 0.5) / 10000.0;
}
static double rd_lambda2(int qp)
{
    double v = floor(0.038 * exp(0.234 * (double)qp) * 10000.0) / 10000.0;
    return v * (double)(1 << (2 * (X265AMD_DEPTH - 8)));
}

extern "C" void x265amd_rdcost(int qp, int sliceType, double psyRdScale, uint64_t dist, uint32_t bits, uint32_t psycost, uint64_t* out)
{
    static const uint32_t psyScaleFix8[3] = { 300, 256, 96 };      /* B, P, I */
    uint64_t lambda2 = (uint64_t)floor(256.0 * rd_lambda2(qp)), lambda = (uint64_t)floor(256.0 * rd_lambda(qp));
    uint32_t psyRdBase = (uint32_t)floor(65536.0 * psyRdScale * 0.33);
    uint32_t psyRd = (psyRdBase * psyScaleFix8[sliceType]) >> 8;
    if (qp >= 40)
    {
        int scale = qp >= 51 ? 0 : (51 - qp) * 23;
        psyRd = (psyRd * scale) >> 8;
    }
    out[0] = lambda2; out[1] = lambda; out[2] = psyRd;
    out[3] = dist + ((bits * lambda2 + 128) >> 8);
    out[4] = psyRd ? dist + ((lambda * psyRd * psycost) >> 24) + ((bits * lambda2) >> 8) : 0;
    out[5] = dist + ((bits * lambda + 128) >> 8);
}
