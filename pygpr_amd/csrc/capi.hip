// extern "C" surface of libpygpr_hip (declared in include/pygpr_hip.h): argument checks, dtype dispatch.
#include "gemm.h"
#include "kbuild.h"
#include "leaf.h"
#include "chainstep.h"
#include "linalg.h"
#include "pygpr_hip_loo.h"
#include "pygpr_hip_sample.h"
#include "sparse.h"
#include "select.h"
#include "kmatmul.h"
#include "dmatmul.h"
#include "krowsq.h"
#include "fmatmul.h"
#include "lowrank.h"
#include "lxgrad.h"
#include "vecchia.h"
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

static thread_local char g_err[512] = "";

// Live handles.  A handle owns priority / CU-masked streams and events; if they are still alive when the HIP runtime
// tears itself down at process exit, the runtime's finalisers touch freed queue state (round 1: SIGSEGV in
// __cxa_finalize under rocprofv3, after the profiler had written its output).  pg_create therefore registers a C atexit
// handler the first time it runs -- i.e. after the HIP runtime registered its own, so it runs BEFORE the runtime's --
// that destroys whatever the caller did not pg_destroy.
static std::mutex g_live_mu;
static std::vector<pg_ctx*> g_live;
static bool g_atexit_registered = false;

static void release_ctx(pg_ctx* h) {
    (void)hipStreamDestroy(h->aux);
    if (h->rows) (void)hipStreamDestroy(h->rows);
    if (h->upd) (void)hipStreamDestroy(h->upd);
    for (int i = 0; i < 8; ++i) (void)hipEventDestroy(h->ev[i]);
    for (int i = 0; i < h->npool; ++i) (void)hipEventDestroy(h->pool[i]);
    free(h->pool);
    if (h->tmo_host) (void)hipHostFree(h->tmo_host);
    if (h->probe_words) (void)hipHostFree(h->probe_words);
    delete h;
}

static void destroy_live_handles() {
    std::vector<pg_ctx*> left;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        left.swap(g_live);
    }
    if (left.empty()) return;
    (void)hipDeviceSynchronize();
    for (pg_ctx* h : left) release_ctx(h);
}

void pg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define NEED(cond, what)                                         \
    do {                                                         \
        if (!(cond)) { pg_set_error("%s: %s", __func__, what); return -1; } \
    } while (0)
// The GEMM core, the chain kernels, the covariance tiles, the gradient bodies and the triangular mat-vecs move 16-byte words
// (vec_t) at base + r * ld + c with c a multiple of the vector width: every operand they touch needs a 16-byte aligned base and
// 16-byte rows (and expert strides).  Checked here, before anything is enqueued; scalar kernels (pg_tril, pg_symmetrize, pg_logdet,
// pg_nlml_value, the committee's element-wise entry points, pg_sqdist_argmin, pg_kernel_grad_build, pg_kernel_xgrad, pg_chol_append)
// take any ld >= width.
static bool rows16(int dtype, const void* p, long ld) {
    const long e = dtype == PG_F32 ? 4 : 8;
    return !p || (reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * e) % 16 == 0);      // (a NULL operand is optional: nothing to align)
}
#define NEED16(p, ld) NEED(rows16(dtype, (p), (ld)), #p ": base and rows (" #ld ") must be 16-byte aligned")
#define NEEDS16(p, stride) NEED(!(p) || ((stride) * (dtype == PG_F32 ? 4 : 8)) % 16 == 0, #p ": expert stride " #stride " must keep every expert 16-byte aligned")
// dtype dispatch: `call` is a generic lambda that receives a double or a float and names its type T.  `fn` is the entry point's name,
// passed in by the caller (__func__ inside the lambda would name the lambda).
template <typename F>
static int dispatch(int dtype, const char* fn, F&& call) {
    if (dtype == PG_F64) return call(double());
    if (dtype == PG_F32) return call(float());
    pg_set_error("%s: unknown dtype %d", fn, dtype);
    return -1;
}

// A timed-out wait of the coupled chain (chainstep.h) sets the handle's pinned host word: from the next entry point on the handle
// factorises on the classic chain (no flags, no resident kernels), so that repeating the failed call -- which is what
// pg_build_potrf_trtri_checked and the Python layer do -- ends in a correct factor.  pg_set_coupled_chain(h, 1) probes and re-arms.
static void poll_timeout(pg_ctx* h) {
    if (h && h->tmo_host) {
        const int v = *(volatile int*)h->tmo_host;     // epoch of the factorisation whose wait expired (chainstep.h)
        if (v) {
            *(volatile int*)h->tmo_host = 0;
            if (h->coupled) {
                h->tmo_off = 1; h->calls_since_tmo = 0;
                if (h->rearms > h->rearms_seen) { h->rearm_cur = std::min(4096, std::max(1, h->rearm_cur) * 2); h->rearms_seen = h->rearms; }   // timed out again after a re-arm: back off
            }
            h->coupled = 0;
            if (v != h->counted_epoch) {               // one count per call, however many waits expired and whenever we looked
                h->counted_epoch = v;
                h->timeouts += 1;
            }
        }
    }
}

// pg_alpha_nlml_async leaves work on the handle's side stream; every entry point that may read its outputs (everything that
// takes a stream except pg_lauum, which is meant to overlap with it) first makes its stream wait for that work.  Only a join on
// the stream the work was forked from retires the pending mark: a call on another stream in between waits too, but the owner's
// next reader still does (round 2 cleared the mark at the first join of ANY stream).
static int join_side(pg_ctx* h, void* stream) {
    poll_timeout(h);
    if (h && h->side_pending) {
        PG_CHECK(hipStreamWaitEvent(ST(stream), h->ev[5], 0));
        if (ST(stream) == h->side_owner) h->side_pending = 0;
    }
    return 0;
}
#define JOIN(h, stream)                         \
    do {                                        \
        int _j = join_side((h), (stream));      \
        if (_j) return _j;                      \
    } while (0)

// The beta == 1 epilogue of the GEMM core adds into C with no-return fp64 atomics performed at the memory side.  On fine-grained,
// host-pinned or managed allocations such atomics may be dropped or crawl, so the entry points that take a caller-owned C check
// the pointer once and keep the read-modify-write epilogue for anything that is not plain device memory.
static int plain_device_memory(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    // (fine-grained device allocations -- hipExtMallocWithFlags(hipDeviceMallocFinegrained) -- also report hipMemoryTypeDevice: they are
    //  exactly the memory where memory-side fp64 atomics may be dropped)
    return a.type == hipMemoryTypeDevice && !a.isManaged && !(a.allocationFlags & hipDeviceMallocFinegrained);
}
struct AtomicGuard {
    pg_ctx* h;
    AtomicGuard(pg_ctx* h_, const void* c) : h(h_) { if (h) h->no_atomic_c = plain_device_memory(c) ? 0 : 1; }
    ~AtomicGuard() { if (h) h->no_atomic_c = 0; }
};

template <typename T>
static int gemm_raw_t(pg_handle h, int variant, int M, int N, int K, double alpha, const void* A, long lda, const void* B,
                      long ldb, double beta, void* C, long ldc, int tri, int klo, int khi, void* stream) {
    GemmP<T> p;
    p.A = (const T*)A; p.B = (const T*)B; p.C = (T*)C;
    p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.M = M; p.N = N; p.K = K;
    p.alpha = (T)alpha; p.beta = (T)beta;
    p.klo = klo & 3; p.khi = khi; p.krev = (klo >> 2) & 1;   // (klo bit 2: reverse walk, measurement only)
    p.exact = (klo >> 3) & 1;                                             // (klo bit 3: the variant's own form, no routing -- measurement only)
    p.sA = p.sB = p.sC = 0; p.batch = 1;
    p.nexp = 1; p.eA = p.eB = p.eC = 0; p.einfo = 0;
    p.part = nullptr; p.ldp = 0; p.info = nullptr; p.noxcd = 0;
    // tri bits 1 - 3 (tests only: the levels of a launch that the call has no arguments for).  2: batch = 2, 4: nexp = 2 -- the problems lie
    // stacked, each array's next block right below the previous one (experts outermost); 8: the launch has status flags, one int per
    // expert, at the 16 bytes in front of C.
    p.tri = tri & 1;
    if (tri & 14) {
        const bool ta = variant == GEMM_TN_128 || variant == GEMM_TT_128 || variant == GEMM_TT_64 || variant == GEMM_TN_64 ||
                        variant == GEMM_TN_128_PL || variant == GEMM_TT_128_PL;
        const bool tb = !(variant == GEMM_NN_128 || variant == GEMM_TN_128 || variant == GEMM_TN_64 || variant == GEMM_NN_128_PL ||
                          variant == GEMM_TN_128_PL);
        p.batch = (tri & 2) ? 2 : 1;
        p.nexp = (tri & 4) ? 2 : 1;
        p.sA = (long)(ta ? K : M) * lda; p.sB = (long)(tb ? N : K) * ldb; p.sC = (long)M * ldc;
        p.eA = p.batch * p.sA; p.eB = p.batch * p.sB; p.eC = p.batch * p.sC;
        if (tri & 8) { p.info = reinterpret_cast<const int*>(reinterpret_cast<const char*>(C) - 16); p.einfo = 1; }
    }
    // PG_RAW_STREAM=upd (measurement only): run the product on the handle's CU-masked update stream instead
    static const char* rs = getenv("PG_RAW_STREAM");
    hipStream_t on = ST(stream);
    if (rs && rs[0] == 'u' && h->upd) on = h->upd;
    if (on == ST(stream)) return pg_gemm<T>(h, on, variant, p);
    PG_CHECK(hipEventRecord(h->ev[2], ST(stream)));      // (ev[4] / ev[5] belong to pg_alpha_nlml_async's side-stream fork)
    PG_CHECK(hipStreamWaitEvent(on, h->ev[2], 0));
    const int rc = pg_gemm<T>(h, on, variant, p);
    PG_CHECK(hipEventRecord(h->ev[3], on));
    PG_CHECK(hipStreamWaitEvent(ST(stream), h->ev[3], 0));
    return rc;
}

// Do kernels of the panel stream and the rows stream run at the same time here?  The coupled chain needs that: its leaf is
// resident while the rows kernel that publishes its tile is still queued on the other stream.  A counter-collecting profiler
// (rocprofv3 --pmc) or a serialising debug setting runs one kernel at a time; the chain's bounded waits would then expire and the
// factorisation report info = -1.  Probe once per handle: a waiter on the panel stream, enqueued FIRST, then the setter on the rows
// stream.  Concurrent queues: the waiter sees the flag within microseconds.  One kernel at a time: it gives up after ~2 ms.
__global__ void pg_probe_wait_kernel(int* flag, int* seen) {
    int ok = 0;
    for (int it = 0; it < 4096 && !ok; ++it) {
        ok = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
        __builtin_amdgcn_s_sleep(32);
    }
    __hip_atomic_store(seen, ok ? 1 : 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void pg_probe_set_kernel(int* flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

static int probe_concurrent_queues(pg_ctx* c) {
    // (the words live as long as the handle: a re-arm inside an enqueueing entry point then costs the probe's two stream
    //  synchronisations, not a pinned allocation and its device-wide release as well)
    if (!c->probe_words && hipHostMalloc(reinterpret_cast<void**>(&c->probe_words), 64, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        c->probe_words = nullptr;
        return 0;
    }
    int* words = c->probe_words;
    words[0] = 0;
    words[1] = 0;
    int* dwords = nullptr;
    int ok = 0;
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&dwords), words, 0) == hipSuccess) {
        hipLaunchKernelGGL(pg_probe_wait_kernel, dim3(1), dim3(1), 0, c->aux, dwords, dwords + 1);
        hipLaunchKernelGGL(pg_probe_set_kernel, dim3(1), dim3(1), 0, c->rows, dwords);
        if (hipStreamSynchronize(c->aux) == hipSuccess && hipStreamSynchronize(c->rows) == hipSuccess) ok = words[1] == 1;
    }
    (void)hipGetLastError();
    return ok;
}

// A handle whose chain was switched off by a time-out counts its factorisations; after rearm_after of them it probes the queues
// again (2 ms at most, once) and takes the coupled chain back: the cause on record (profiles/r03_bench_n2_gloo_rehearsal.json: another
// process's resident kernels on the same GPU) is transient, the downgrade should be too.
static void maybe_rearm(pg_ctx* h) {
    if (h && h->coupled && h->rearms > 0 && h->rearm_cur > h->rearm_after && ++h->calls_since_rearm > h->rearm_cur) {
        h->rearm_cur = h->rearm_after;      // the re-armed chain ran cleanly for a whole back-off distance: forget the back-off
        h->calls_since_rearm = 0;
    }
    if (!h || !h->tmo_off || h->coupled || h->rearm_after <= 0) return;
    if (h->rearm_cur < h->rearm_after) h->rearm_cur = h->rearm_after;
    if (++h->calls_since_tmo <= h->rearm_cur) return;
    h->calls_since_tmo = 0;
    if (h->rows && h->spin_ticks >= 0 && probe_concurrent_queues(h)) {
        h->coupled = 1;
        h->tmo_off = 0;
        h->rearms += 1;
        h->calls_since_rearm = 0;
    }
}

template <typename T>
static int build_potrf_t(pg_handle h, hipStream_t st, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d,
                         double jitter, void* A, long lda, int n_pad, void* inv_diag, int* info, void* Minv, long ldm) {
    BuildReq<T> br;
    br.spec = spec; br.hp = hp; br.X = (const T*)X; br.ldx = ldx; br.n_real = n; br.d = d; br.jitter = jitter;
    return pg_potrf_t<T>(h, st, n_pad, (T*)A, lda, (T*)inv_diag, info, (T*)Minv, ldm, &br);
}

template <typename T>
static int potrf_batched_t(pg_handle h, hipStream_t st, const pg_covspec* spec, const double* hp, long hp_stride, const void* X, long ldx,
                           long x_stride, int n, int d, double jitter, void* A, long lda, long a_stride, int n_pad, void* inv_diag,
                           long inv_stride, int* info, void* Minv, long ldm, long m_stride, int nexp) {
    ExpBatch eb;
    eb.nexp = nexp; eb.eA = a_stride; eb.eInv = inv_stride; eb.eM = m_stride; eb.eX = x_stride; eb.ehp = hp_stride;
    BuildReq<T> br;
    br.spec = spec; br.hp = hp; br.X = (const T*)X; br.ldx = ldx; br.n_real = n; br.d = d; br.jitter = jitter;
    return pg_potrf_t<T>(h, st, n_pad, (T*)A, lda, (T*)inv_diag, info, (T*)Minv, ldm, X ? &br : nullptr, &eb);
}

extern "C" {

int pg_version(void) { return 100; }
const char* pg_last_error(void) { return g_err; }

int pg_create(pg_handle* h) {
    NEED(h, "null handle pointer");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        pg_set_error("pg_create: no HIP device visible");
        return -101;
    }
    pg_ctx* c = new pg_ctx();
    memset(c, 0, sizeof(*c));
    int prio_lo = 0, prio_hi = 0;
    PG_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    PG_CHECK(hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, prio_hi));
    c->rows = nullptr;
    c->last_coupled = 0;
    c->lookahead = 1;
    {
        const char* e = getenv("PG_NBO");
        c->nbo = e ? atoi(e) : 0;
        if (c->nbo < 128 || c->nbo % 128 || c->nbo > 2048) c->nbo = 0;
        const char* r = getenv("PG_REC_MIN");
        c->rec_min = r ? atoi(r) : 16384;
        if (c->rec_min < 0 || (c->rec_min > 0 && (c->rec_min < 512 || c->rec_min % 512))) c->rec_min = 16384;
    }
    {   // update stream on all but the last PG_RESERVED_CUS compute units; without it look-ahead stays off
        hipDeviceProp_t prop;
        int dev = 0;
        PG_CHECK(hipGetDevice(&dev));
        PG_CHECK(hipGetDeviceProperties(&prop, dev));
        const int ncu = prop.multiProcessorCount;
        const int words = (ncu + 31) / 32;
        uint32_t mask[64];
        for (int i = 0; i < 64; ++i) mask[i] = 0;
        const char* env = getenv("PG_RESERVED_CUS");
        int reserved = env ? atoi(env) : PG_RESERVED_CUS;
        if (reserved < 1 || reserved > ncu / 2) reserved = PG_RESERVED_CUS;
        c->ncu = ncu; c->upd_cus = ncu - reserved;
        for (int cu = 0; cu < ncu - reserved; ++cu) mask[cu / 32] |= (1u << (cu % 32));   // (a strided reservation was measured: 9 % slower)
        if (ncu <= reserved * 2 || words > 64 ||
            hipExtStreamCreateWithCUMask(&c->upd, (uint32_t)words, mask) != hipSuccess) {
            c->upd = nullptr;
            c->lookahead = 0;
            (void)hipGetLastError();
        }
    }
    {   // rows stream of the flag-coupled chain (chainstep.hip): non-blocking, same priority as the panel stream
        const char* envr = getenv("PG_ROWS_STREAM");
        c->rows = nullptr;
        if (!(envr && !atoi(envr)) && c->upd &&
            hipStreamCreateWithPriority(&c->rows, hipStreamNonBlocking, prio_hi) != hipSuccess) {
            c->rows = nullptr;
            (void)hipGetLastError();
        }
    }
    c->coupled = (c->rows && probe_concurrent_queues(c)) ? 1 : 0;
    {   // pinned word through which a timed-out wait of the coupled chain reaches the host (poll_timeout), and the wait budget
        c->tmo_host = nullptr;
        c->tmo_dev = nullptr;
        if (hipHostMalloc(reinterpret_cast<void**>(&c->tmo_host), 64, hipHostMallocMapped) == hipSuccess) {
            c->tmo_host[0] = 0;
            if (hipHostGetDevicePointer(reinterpret_cast<void**>(&c->tmo_dev), c->tmo_host, 0) != hipSuccess) c->tmo_dev = nullptr;
        }
        (void)hipGetLastError();
        // budget of one wait: by default scaled to the call (pg_potrf_t: 20x the classic-chain estimate of the coupled region, at least
        // 50 ms -- round 3's flat 2 s was 70x a whole N = 16384 factorisation, and in a lock-step all-reduce one rank's stall is every
        // rank's); PG_CS_SPIN_US / pg_set_spin_budget fix it
        const char* e = getenv("PG_CS_SPIN_US");
        const long long us = e ? atoll(e) : 0;
        c->spin_ticks = us < 0 ? -1 : us * 100;
        c->timeouts = 0;
        const char* ra = getenv("PG_CS_REARM");
        c->rearm_after = ra ? std::max(0, atoi(ra)) : 8;
        c->rearm_cur = c->rearm_after;
    }
    for (int i = 0; i < 8; ++i) PG_CHECK(hipEventCreate(&c->ev[i]));
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.push_back(c);
        if (!g_atexit_registered) {
            atexit(destroy_live_handles);
            g_atexit_registered = true;
        }
    }
    *h = c;
    return 0;
}

int pg_destroy(pg_handle h) {
    if (!h) return 0;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        auto it = std::find(g_live.begin(), g_live.end(), h);
        if (it == g_live.end()) return 0;      // already released (second pg_destroy, or after the exit handler ran)
        g_live.erase(it);
    }
    release_ctx(h);
    return 0;
}

// A product spec (PG_SPEC_PRODUCT or-ed into ncomp) holds 1..PG_MAX_COMP factors and never PG_KIND_SQDIST; an unflagged spec is checked
// as it always was.  The flag itself is stripped further down (pg_spec_strip, kbuild.h), by every host routine that takes a spec.
static int check_spec(const pg_covspec* s, const char* fn, bool allow_sqdist = false) {
    const bool prod = s && s->ncomp >= 0 && (s->ncomp & PG_SPEC_PRODUCT);
    const int ncomp = !s ? 0 : (prod ? (s->ncomp ^ PG_SPEC_PRODUCT) : s->ncomp);
    if (prod && (ncomp < 1 || ncomp > PG_MAX_COMP)) {
        pg_set_error("%s: a product spec needs 1..%d factors, got %d", fn, PG_MAX_COMP, ncomp);
        return -1;
    }
    if (prod) allow_sqdist = false;
    if (!s || ncomp < 0 || ncomp > PG_MAX_COMP || s->nnoise < 0 || s->nnoise > PG_MAX_COMP) {
        pg_set_error("%s: bad covariance spec", fn);
        return -1;
    }
    for (int c = 0; c < ncomp; ++c)
        if (s->kind[c] != PG_KIND_RBF && s->kind[c] != PG_KIND_MATERN52 && s->kind[c] != PG_KIND_MATERN32 && s->kind[c] != PG_KIND_MATERN12 &&
            s->kind[c] != PG_KIND_RQ && s->kind[c] != PG_KIND_PERIODIC && !(allow_sqdist && s->kind[c] == PG_KIND_SQDIST)) {
            pg_set_error("%s: unknown kernel kind %d", fn, s->kind[c]);
            return -1;
        }
    return 0;
}

int pg_kernel_build(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr,
                    const void* Xc, long ldc, int nc, int d, int lower_only, int accumulate, double jitter, void* K,
                    long ldk, int rows_pad, int cols_pad, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && Xr && K, "null pointer");
    if (check_spec(spec, __func__, true)) return -1;
    const int sym = (Xc == nullptr);
    if (sym) { Xc = Xr; ldc = ldr; nc = nr; }
    NEED(nr >= 0 && nc >= 0 && rows_pad >= nr && cols_pad >= nc && ldk >= cols_pad, "inconsistent sizes");
    NEED(!sym || rows_pad == cols_pad, "symmetric build needs a square padded shape");
    NEED(ldk % (dtype == PG_F64 ? 2 : 4) == 0, "ldk must keep rows 16-byte aligned");
    NEED16(K, ldk);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_kbuild<T>(ST(stream), *spec, hp, (const T*)Xr, ldr, nr, (const T*)Xc, ldc, nc, d, sym, lower_only, accumulate, jitter,
                            (T*)K, ldk, rows_pad, cols_pad);
    });
}

int pg_kernel_build_batched(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, long hp_stride, const void* Xr, long ldr,
                            long xr_stride, int nr, const void* Xc, long ldc, long xc_stride, int nc, int d, int lower_only, double jitter,
                            void* K, long ldk, long k_stride, int rows_pad, int cols_pad, int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && Xr && K, "null pointer");
    if (check_spec(spec, __func__, true)) return -1;
    NEED(nexp >= 1 && nexp <= 65535, "1 <= nexp <= 65535");
    const int sym = (Xc == nullptr);
    if (sym) { Xc = Xr; ldc = ldr; nc = nr; xc_stride = xr_stride; }
    NEED(nr >= 0 && nc >= 0 && rows_pad >= nr && cols_pad >= nc && ldk >= cols_pad, "inconsistent sizes");
    NEED(!sym || rows_pad == cols_pad, "symmetric build needs a square padded shape");
    NEED(nexp == 1 || k_stride >= (long)rows_pad * ldk, "experts' matrices overlap");
    NEED(ldk % (dtype == PG_F64 ? 2 : 4) == 0, "ldk must keep rows 16-byte aligned");
    NEED16(K, ldk); NEEDS16(K, k_stride);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_kbuild<T>(ST(stream), *spec, hp, (const T*)Xr, ldr, nr, (const T*)Xc, ldc, nc, d, sym, lower_only, 0, jitter, (T*)K, ldk,
                            rows_pad, cols_pad, 0, 0, nexp, xc_stride, hp_stride, k_stride, xr_stride);
    });
}

int pg_kernel_grad_build(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx,
                         int n, int d, void* dK, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && X && dK, "null pointer");
    if (check_spec(spec, __func__)) return -1;
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_kgrad<T>(ST(stream), *spec, hp, (const T*)X, ldx, n, d, (T*)dK);
    });
}

int pg_build_potrf_trtri(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d,
                         double jitter, void* A, long lda, int n_pad, void* inv_diag, int* info, void* Minv, long ldm,
                         void* stream) {
    JOIN(h, stream);
    maybe_rearm(h);
    NEED(h && hp && X && A && inv_diag && info, "null pointer");
    if (check_spec(spec, __func__, true)) return -1;
    NEED(n >= 0 && n_pad >= n && lda >= n_pad, "inconsistent sizes");
    NEED(lda % (dtype == PG_F64 ? 2 : 4) == 0, "lda must keep rows 16-byte aligned");
    NEED16(A, lda); NEED16(inv_diag, 0); NEED16(Minv, ldm);
    AtomicGuard ag(h, A);
    return dispatch(dtype, __func__, [&](auto t) {
        return build_potrf_t<decltype(t)>(h, ST(stream), spec, hp, X, ldx, n, d, jitter, A, lda, n_pad, inv_diag, info, Minv, ldm);
    });
}

int pg_build_potrf_trtri_batched(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, long hp_stride, const void* X, long ldx,
                                 long x_stride, int n, int d, double jitter, void* A, long lda, long a_stride, int n_pad, void* inv_diag,
                                 long inv_stride, int* info, void* Minv, long ldm, long m_stride, int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && A && inv_diag && info, "null pointer");
    NEED(!X || hp, "a folded build needs hp");
    if (X && check_spec(spec, __func__, true)) return -1;
    NEED(nexp >= 1 && nexp <= 65535, "1 <= nexp <= 65535");
    NEED(n >= 0 && n_pad >= n && lda >= n_pad, "inconsistent sizes");
    NEED(a_stride >= (long)n_pad * lda || nexp == 1, "experts' matrices overlap");
    NEED(inv_stride >= pg_potrf_worksize_impl(n_pad) || nexp == 1, "experts' workspaces overlap (stride < pg_potrf_worksize)");
    NEED(!Minv || (ldm >= n_pad && (m_stride >= (long)n_pad * ldm || nexp == 1)), "experts' inverses overlap");
    NEED(lda % (dtype == PG_F64 ? 2 : 4) == 0, "lda must keep rows 16-byte aligned");
    NEED16(A, lda); NEEDS16(A, a_stride); NEED16(inv_diag, inv_stride); NEED16(Minv, ldm); NEEDS16(Minv, m_stride);
    maybe_rearm(h);      // a batched-only workload counts towards the re-arm like the single-matrix calls (one per call)
    AtomicGuard ag(h, A);
    return dispatch(dtype, __func__, [&](auto t) {
        return potrf_batched_t<decltype(t)>(h, ST(stream), spec, hp, hp_stride, X, ldx, x_stride, n, d, jitter, A, lda, a_stride, n_pad, inv_diag,
                                            inv_stride, info, Minv, ldm, m_stride, nexp);
    });
}

long pg_potrf_worksize(int dtype, int n) { (void)dtype; return pg_potrf_worksize_impl(n); }

int pg_potrf(pg_handle h, int dtype, int n, void* A, long lda, void* inv_diag, int* info, void* stream) {
    JOIN(h, stream);
    maybe_rearm(h);
    NEED(h && A && inv_diag && info, "null pointer");
    AtomicGuard ag(h, A);
    NEED(lda >= n, "lda < n");
    NEED16(A, lda); NEED16(inv_diag, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_potrf_t<T>(h, ST(stream), n, (T*)A, lda, (T*)inv_diag, info, nullptr, 0);
    });
}

int pg_potrf_trtri(pg_handle h, int dtype, int n, void* A, long lda, void* inv_diag, int* info, void* Minv, long ldm,
                   void* stream) {
    JOIN(h, stream);
    maybe_rearm(h);
    NEED(h && A && inv_diag && info && Minv, "null pointer");
    NEED(lda >= n && ldm >= n && A != Minv, "bad leading dimension / aliasing");
    NEED16(A, lda); NEED16(inv_diag, 0); NEED16(Minv, ldm);
    AtomicGuard ag(h, A);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_potrf_t<T>(h, ST(stream), n, (T*)A, lda, (T*)inv_diag, info, (T*)Minv, ldm);
    });
}

long pg_potrs_vec_worksize(int dtype, int n) { (void)dtype; return pg_potrs_vec_worksize_impl(n); }

int pg_potrs_vec(pg_handle h, int dtype, int n, const void* L, long ldl, const void* inv_diag, const void* y, void* x,
                 void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && L && inv_diag && y && x && work, "null pointer");
    NEED(ldl >= n, "ldl < n");
    NEED16(L, ldl); NEED16(inv_diag, 0); NEED16(y, 0); NEED16(x, 0); NEED16(work, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_potrs_vec_t<T>(h, ST(stream), n, (const T*)L, ldl, (const T*)inv_diag, (const T*)y, (T*)x, (T*)work);
    });
}

int pg_trtri(pg_handle h, int dtype, int n, const void* L, long ldl, const void* inv_diag, void* Minv, long ldm,
             void* stream) {
    JOIN(h, stream);
    NEED(h && L && inv_diag && Minv, "null pointer");
    NEED(L != Minv, "pg_trtri is out of place");
    NEED(ldl >= n && ldm >= n, "leading dimension < n");
    NEED16(L, ldl); NEED16(inv_diag, 0); NEED16(Minv, ldm);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_trtri_t<T>(h, ST(stream), n, (const T*)L, ldl, (const T*)inv_diag, (T*)Minv, ldm);
    });
}

long pg_potrs_worksize(int dtype, int n, int nrhs, int have_minv) {
    (void)dtype;
    return (have_minv ? 0L : (long)n * n) + (long)n * nrhs;
}

static int potrs_any(pg_handle h, int dtype, int n, int nrhs, const void* L, long ldl, const void* inv_diag, const void* Minv, long ldm,
                     const void* B, long ldb, void* X, long ldx, void* work, int both, void* stream) {
    JOIN(h, stream);
    NEED(h && B && X && work && (Minv || (L && inv_diag)), "null pointer");
    NEED(ldb >= nrhs && ldx >= nrhs && (Minv ? ldm >= n : ldl >= n), "leading dimension too small");
    NEED(B != X, "out of place: X must not alias B");
    NEED16(L, ldl); NEED16(inv_diag, 0); NEED16(Minv, ldm); NEED16(B, ldb); NEED16(X, ldx); NEED16(work, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_potrs_t<T>(h, ST(stream), n, nrhs, (const T*)L, ldl, (const T*)inv_diag, (const T*)Minv, ldm, (const T*)B, ldb, (T*)X, ldx,
                             (T*)work, both);
    });
}
int pg_potrs(pg_handle h, int dtype, int n, int nrhs, const void* L, long ldl, const void* inv_diag, const void* Minv, long ldm, const void* B,
             long ldb, void* X, long ldx, void* work, void* stream) {
    return potrs_any(h, dtype, n, nrhs, L, ldl, inv_diag, Minv, ldm, B, ldb, X, ldx, work, 1, stream);
}
int pg_trsm_lower(pg_handle h, int dtype, int n, int nrhs, const void* L, long ldl, const void* inv_diag, const void* Minv, long ldm,
                  const void* B, long ldb, void* X, long ldx, void* work, void* stream) {
    return potrs_any(h, dtype, n, nrhs, L, ldl, inv_diag, Minv, ldm, B, ldb, X, ldx, work, 0, stream);
}

int pg_lauum(pg_handle h, int dtype, int n, const void* Minv, long ldm, void* Kinv, long ldk, void* stream) {
    NEED(h && Minv && Kinv, "null pointer");
    NEED(Minv != Kinv, "pg_lauum is out of place");
    NEED(ldm >= n && ldk >= n, "leading dimension < n");
    NEED16(Minv, ldm); NEED16(Kinv, ldk);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_lauum_t<T>(h, ST(stream), n, (const T*)Minv, ldm, (T*)Kinv, ldk);
    });
}

int pg_potri(pg_handle h, int dtype, int n, const void* L, long ldl, const void* inv_diag, void* Kinv, long ldk, void* work,
             void* stream) {
    JOIN(h, stream);
    NEED(h && L && inv_diag && Kinv && work, "null pointer");
    NEED(work != L && work != Kinv, "pg_potri: work must not alias L or Kinv");
    NEED(ldl >= n && ldk >= n, "leading dimension < n");
    NEED16(work, 0);
    int rc = pg_trtri(h, dtype, n, L, ldl, inv_diag, work, (long)n, stream);
    if (rc) return rc;
    return pg_lauum(h, dtype, n, work, (long)n, Kinv, ldk, stream);
}

int pg_logdet(pg_handle h, int dtype, int n, const void* L, long ldl, double* out, void* stream) {
    JOIN(h, stream);
    NEED(h && L && out, "null pointer");
    NEED(n > 0 && ldl >= n, "bad size");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_logdet_t<T>(ST(stream), n, (const T*)L, ldl, out);
    });
}

int pg_trmv(pg_handle h, int dtype, int n, const void* Minv, long ldm, int trans, const void* x, void* y, void* work,
            void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && x && y, "null pointer");
    NEED(!trans || work, "transposed product needs a workspace");
    NEED(x != y, "pg_trmv is out of place");
    NEED(ldm >= n, "ldm < n");
    NEED16(Minv, ldm); NEED16(x, 0); NEED16(y, 0); NEED16(work, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_trmv_t<T>(h, ST(stream), n, (const T*)Minv, ldm, trans, (const T*)x, (T*)y, (T*)work);
    });
}

long pg_chol_append_worksize(int dtype, int n_pad, int k) {
    if (dtype != PG_F64 && dtype != PG_F32) return -1;
    return pg_chol_append_worksize_impl(dtype == PG_F64 ? 8 : 4, n_pad, k);
}

int pg_chol_append(pg_handle h, int dtype, int n, int k, int n_pad, void* L, long ldl, void* inv_diag, void* Minv, long ldm, const void* Kt,
                   long ldkt, const void* Knn, long ldknn, const void* y_new, void* u, void* alpha, void* work, int* info, void* stream) {
    JOIN(h, stream);
    NEED(h && L && inv_diag && Minv && Kt && Knn && y_new && u && alpha && work && info, "null pointer");
    NEED(n_pad > 0 && n_pad % PG_PAD == 0, "n_pad must be a positive multiple of 256");
    NEED(k >= 1 && k <= PG_APPEND_KMAX, "1 <= k <= 128");
    NEED(n >= 1 && n + k <= n_pad, "1 <= n and n + k <= n_pad");
    NEED(ldl >= n_pad && ldm >= n_pad, "ldl, ldm >= n_pad");
    NEED(ldkt >= n && ldknn >= k, "ldkt >= n, ldknn >= k");
    NEED(L != Minv && u != alpha, "L / Minv and u / alpha must not alias");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_chol_append_t<T>(h, ST(stream), n, k, n_pad, (T*)L, ldl, (T*)inv_diag, (T*)Minv, ldm, (const T*)Kt, ldkt, (const T*)Knn, ldknn,
                                   (const T*)y_new, (T*)u, (T*)alpha, work, info);
    });
}

long pg_loo_terms_worksize(int n_pad) { return (n_pad > 0 && n_pad % PG_PAD == 0) ? pg_loo_terms_worksize_impl(n_pad) : -1; }

int pg_loo_terms(pg_handle h, int dtype, int n, int n_pad, const void* Minv, long ldm, const void* alpha, const void* y, void* c, void* mu,
                 void* var, double* out, double* work, void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && alpha && y && c && mu && var && out && work, "null pointer");
    NEED(n_pad > 0 && n_pad % PG_PAD == 0, "n_pad must be a positive multiple of 256");
    NEED(n >= 1 && n <= n_pad && ldm >= n_pad, "1 <= n <= n_pad <= ldm");
    NEED16(Minv, ldm);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_loo_terms_t<T>(ST(stream), n, n_pad, (const T*)Minv, ldm, (const T*)alpha, (const T*)y, (T*)c, (T*)mu, (T*)var, out, work);
    });
}

int pg_loo_weights(pg_handle h, int dtype, int n, const void* c, const void* alpha, void* Kinv, long ldk, void* p, void* q, void* stream) {
    JOIN(h, stream);
    NEED(h && c && alpha && Kinv && p && q, "null pointer");
    NEED(n >= 1 && ldk >= n, "1 <= n <= ldk");
    NEED(p != q && p != c && p != alpha && q != c && q != alpha, "p and q must not alias each other, c or alpha");
    NEED16(Kinv, ldk);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_loo_weights_t<T>(ST(stream), n, (const T*)c, (const T*)alpha, (T*)Kinv, ldk, (T*)p, (T*)q);
    });
}

int pg_loo_fold(pg_handle h, int dtype, int n, void* M, long ldm, const void* q, void* stream) {
    JOIN(h, stream);
    NEED(h && M && q, "null pointer");
    NEED(n >= 1 && ldm >= n, "1 <= n <= ldm");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_loo_fold_t<T>(ST(stream), n, (T*)M, ldm, (const T*)q);
    });
}

long pg_kernel_cross_grad_worksize(int m, int n, int nhp) { return (m >= 0 && n >= 0 && nhp >= 0) ? pg_cross_grad_worksize_impl(m, n, nhp) : -1; }

int pg_kernel_cross_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Z, long ldz, int m, const void* X,
                         long ldx, int n, int d, const void* W, long ldw, double* grad, int accumulate, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && Z && X && W && grad && work, "null pointer");
    if (check_spec(spec, __func__)) return -1;
    if (!(m >= 0 && n >= 0 && d >= 1 && d <= PG_MAX_DIM)) { pg_set_error("%s: bad shape (0 <= m, n; 1 <= d <= PG_MAX_DIM)", __func__); return -2; }
    if ((m + 63) / 64 > 65535) { pg_set_error("%s: m <= 64 * 65535", __func__); return -2; }
    NEED(ldz >= d && ldx >= d && ldw >= n, "ldz, ldx >= d and ldw >= n");
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_cross_grad_t<T>(ST(stream), *spec, hp, (const T*)Z, ldz, m, (const T*)X, ldx, n, d, (const T*)W, ldw, grad, accumulate,
                                  (double*)work);
    });
}

long pg_greedy_select_worksize(int n, int m_max) { return (n >= 0 && m_max >= 0 && m_max <= n) ? pg_greedy_select_worksize_impl(n, m_max) : -1; }

int pg_greedy_select(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d, int m_max,
                     double floor, int* piv, int* count, double* trace, double* resid, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && count, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (check_spec(spec, __func__)) return -1;
    NEED((spec->ncomp & ~PG_SPEC_PRODUCT) >= 1, "the spec has no stationary component");
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    if (!(n >= 0 && d >= 1 && d <= PG_MAX_DIM && m_max >= 0 && m_max <= n)) {
        pg_set_error("%s: bad shape (0 <= m_max <= n; 1 <= d <= PG_MAX_DIM)", __func__);
        return -2;
    }
    NEED(ldx >= d, "ldx >= d");
    NEED(m_max == 0 || (X && piv && trace && resid && work), "null pointer");
    return pg_greedy_select_impl(ST(stream), *spec, hp, (const double*)X, ldx, n, d, m_max, floor, piv, count, trace, resid, (double*)work);
}

long pg_kernel_matmul_worksize(int nr, int nc, int nrhs) { return (nr >= 0 && nc >= 0 && nrhs >= 0) ? pg_kmatmul_worksize_impl(nr, nc, nrhs) : -1; }

int pg_kernel_matmul(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                     long ldc, int nc, int d, const void* V, long ldv, int nrhs, double jitter, void* OUT, long ldo, void* work,
                     void* stream) {
    JOIN(h, stream);
    NEED(h && hp, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (check_spec(spec, __func__)) return -1;      // (PG_KIND_SQDIST is refused: it is no covariance)
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    for (int q = 0; q < spec->nnoise; ++q) NEED(spec->noise_off[q] >= 0, "negative offset in the covariance spec");
    const int sym = (Xc == nullptr);
    if (sym) { Xc = Xr; ldc = ldr; nc = nr; }
    if (!(nr >= 0 && nc >= 0 && nrhs >= 0 && d >= 1 && d <= PG_MAX_DIM)) {
        pg_set_error("%s: bad shape (0 <= nr, nc, nrhs; 1 <= d <= PG_MAX_DIM)", __func__);
        return -2;
    }
    if ((nrhs + 31) / 32 > 65535) { pg_set_error("%s: nrhs <= 32 * 65535", __func__); return -2; }
    NEED(ldr >= d && ldc >= d && ldv >= nrhs && ldo >= nrhs, "ldr, ldc >= d and ldv, ldo >= nrhs");
    if (nr == 0 || nrhs == 0) return 0;
    NEED(Xr && OUT && (nc == 0 || (Xc && V)), "null pointer");
    NEED(work || pg_kmatmul_worksize_impl(nr, nc, nrhs) == 0, "this shape needs its workspace (pg_kernel_matmul_worksize)");
    return pg_kmatmul_impl(ST(stream), *spec, hp, (const double*)Xr, ldr, nr, (const double*)Xc, ldc, nc, d, sym, (const double*)V, ldv, nrhs,
                           jitter, (double*)OUT, ldo, (double*)work);
}

long pg_kernel_rowsq_worksize(int nr, int nc) { return (nr >= 0 && nc >= 0) ? pg_krowsq_worksize_impl(nr, nc) : -1; }

int pg_kernel_rowsq(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                    long ldc, int nc, int d, void* OUT, long ldo, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && hp, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (check_spec(spec, __func__)) return -1;      // (PG_KIND_SQDIST is refused: it is no covariance)
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    NEED(Xc, "cross form only (Xc must not be NULL; it may be Xr)");
    if (!(nr >= 0 && nc >= 0 && d >= 1 && d <= PG_MAX_DIM)) {
        pg_set_error("%s: bad shape (0 <= nr, nc; 1 <= d <= PG_MAX_DIM)", __func__);
        return -2;
    }
    NEED(ldr >= d && ldc >= d && ldo >= 1, "ldr, ldc >= d and ldo >= 1");
    if (nr == 0) return 0;
    NEED(Xr && OUT, "null pointer");
    NEED(work || pg_krowsq_worksize_impl(nr, nc) == 0, "this shape needs its workspace (pg_kernel_rowsq_worksize)");
    return pg_krowsq_impl(ST(stream), *spec, hp, (const double*)Xr, ldr, nr, (const double*)Xc, ldc, nc, d, (double*)OUT, ldo, (double*)work);
}

long pg_kernel_matmul_dx_worksize(int nr, int nc, int d, int nrhs) {
    return (nr >= 0 && nc >= 0 && d >= 0 && nrhs >= 0) ? pg_dmatmul_worksize_impl(nr, nc, d, nrhs) : -1;
}

int pg_kernel_matmul_dx(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                        long ldc, int nc, int d, const void* V, long ldv, int nrhs, void* OUT, long ldo, long ldk, void* work,
                        void* stream) {
    JOIN(h, stream);
    NEED(h && hp, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (check_spec(spec, __func__)) return -1;      // (PG_KIND_SQDIST is refused: it is no covariance)
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    NEED(Xc, "cross form only (Xc must not be NULL; it may be Xr)");
    if (!(nr >= 0 && nc >= 0 && nrhs >= 0 && d >= 1 && d <= PG_MAX_DIM)) {
        pg_set_error("%s: bad shape (0 <= nr, nc, nrhs; 1 <= d <= PG_MAX_DIM)", __func__);
        return -2;
    }
    if ((long)((nrhs + 31) / 32) * dmm_nchunk(d) > 65535) { pg_set_error("%s: nrhs <= 32 * (65535 / chunks of d)", __func__); return -2; }
    NEED(ldr >= d && ldc >= d && ldv >= nrhs && ldk >= nrhs && ldo >= (long)d * ldk, "ldr, ldc >= d, ldv, ldk >= nrhs and ldo >= d * ldk");
    if (nr == 0 || nrhs == 0) return 0;
    NEED(Xr && OUT && (nc == 0 || V), "null pointer");
    NEED(work || pg_dmatmul_worksize_impl(nr, nc, d, nrhs) == 0, "this shape needs its workspace (pg_kernel_matmul_dx_worksize)");
    return pg_dmatmul_impl(ST(stream), *spec, hp, (const double*)Xr, ldr, nr, (const double*)Xc, ldc, nc, d, (const double*)V, ldv, nrhs,
                           (double*)OUT, ldo, ldk, (double*)work);
}

long pg_feature_matmul_worksize(int nr, int nf, int nrhs) { return (nr >= 0 && nf >= 0 && nrhs >= 0) ? pg_fmatmul_worksize_impl(nr, nf, nrhs) : -1; }

int pg_feature_matmul(pg_handle h, int dtype, const void* X, long ldx, int nr, const void* NU, long ldn, int nf, int d, const void* U,
                      const void* W, long ldw, int nrhs, void* OUT, long ldo, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (!(nr >= 0 && nf >= 0 && nrhs >= 0 && d >= 1 && d <= PG_MAX_DIM)) {
        pg_set_error("%s: bad shape (0 <= nr, nf, nrhs; 1 <= d <= PG_MAX_DIM)", __func__);
        return -2;
    }
    if ((nrhs + 31) / 32 > 65535) { pg_set_error("%s: nrhs <= 32 * 65535", __func__); return -2; }
    NEED(ldx >= d && ldn >= d && ldw >= nrhs && ldo >= nrhs, "ldx, ldn >= d and ldw, ldo >= nrhs");
    if (nr == 0 || nrhs == 0) return 0;
    NEED(X && OUT && (nf == 0 || (NU && U && W)), "null pointer");
    NEED(work || pg_fmatmul_worksize_impl(nr, nf, nrhs) == 0, "this shape needs its workspace (pg_feature_matmul_worksize)");
    return pg_fmatmul_impl(ST(stream), (const double*)X, ldx, nr, (const double*)NU, ldn, nf, d, (const double*)U, (const double*)W, ldw, nrhs,
                           (double*)OUT, ldo, (double*)work);
}

long pg_kernel_lowrank_grad_worksize(int nr, int nc, int r, int nhp) {
    return (nr >= 0 && nc >= 0 && r >= 0 && nhp >= 0) ? pg_lowrank_grad_worksize_impl(nr, nc, r, nhp) : -1;
}

int pg_kernel_lowrank_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                           long ldc, int nc, int d, const void* U, long ldu, const void* V, long ldv, int r, double* grad, int accumulate,
                           void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && grad, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (check_spec(spec, __func__)) return -1;      // (PG_KIND_SQDIST is refused: it is no covariance)
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    const int sym = (Xc == nullptr);
    if (sym) { Xc = Xr; ldc = ldr; nc = nr; }
    if (!(nr >= 0 && nc >= 0 && d >= 1 && d <= PG_MAX_DIM)) { pg_set_error("%s: bad shape (0 <= nr, nc; 1 <= d <= PG_MAX_DIM)", __func__); return -2; }
    NEED(r >= 0 && r <= 64, "0 <= r <= 64 (split a larger rank and accumulate)");
    NEED(ldr >= d && ldc >= d && ldu >= r && ldv >= r, "ldr, ldc >= d and ldu, ldv >= r");
    const long size = pg_lowrank_grad_worksize_impl(nr, nc, r, 1);
    NEED(size == 0 || (Xr && Xc && U && V), "null pointer");
    NEED(size == 0 || work, "this shape needs its workspace (pg_kernel_lowrank_grad_worksize)");
    return pg_lowrank_grad_impl(ST(stream), *spec, hp, (const double*)Xr, ldr, nr, (const double*)Xc, ldc, nc, d, sym, (const double*)U, ldu,
                                (const double*)V, ldv, r, grad, accumulate, (double*)work);
}

long pg_kernel_lowrank_xgrad_worksize(int nr, int nc, int d, int r) {
    return (nr >= 0 && nc >= 0 && d >= 0 && r >= 0) ? pg_lxgrad_worksize_impl(nr, nc, d, r) : -1;
}

int pg_kernel_lowrank_xgrad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                            long ldc, int nc, int d, const void* U, long ldu, const void* V, long ldv, int r, void* OUT, long ldo,
                            int accumulate, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && hp, "null pointer");
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (check_spec(spec, __func__)) return -1;      // (PG_KIND_SQDIST is refused: it is no covariance)
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) NEED(spec->off[c] >= 0, "negative offset in the covariance spec");
    const int sym = (Xc == nullptr);
    if (sym) { Xc = Xr; ldc = ldr; nc = nr; }
    NEED(nr >= 0 && nc >= 0 && d >= 1 && d <= PG_MAX_DIM, "bad shape (0 <= nr, nc; 1 <= d <= PG_MAX_DIM)");
    NEED(r >= 0 && r <= 64, "0 <= r <= 64 (split a larger rank and accumulate)");
    NEED(ldr >= d && ldc >= d && ldo >= d && ldu >= r && ldv >= r, "ldr, ldc, ldo >= d and ldu, ldv >= r");
    if (nr == 0) return 0;
    NEED(!sym || V || r == 0, "the symmetric form needs V [nr][r] (V must not be NULL)");
    NEED(Xr && OUT, "null pointer");
    const bool empty = nc == 0 || r == 0;
    NEED(empty || (Xc && U && V), "null pointer");
    NEED(work || pg_lxgrad_worksize_impl(nr, nc, d, r) == 0, "this shape needs its workspace (pg_kernel_lowrank_xgrad_worksize)");
    return pg_lxgrad_impl(ST(stream), *spec, hp, (const double*)Xr, ldr, nr, (const double*)Xc, ldc, nc, d, sym, (const double*)U, ldu,
                          (const double*)V, ldv, r, (double*)OUT, ldo, accumulate, (double*)work);
}

int pg_randn(pg_handle h, int dtype, long seed, int stream_id, int row0, int rows, int cols, void* Z, long ldz, int rows_pad, int cols_pad,
             void* stream) {
    JOIN(h, stream);
    NEED(h && Z, "null pointer");
    NEED(rows_pad >= 1 && cols_pad >= 1 && rows >= 0 && rows <= rows_pad && cols >= 0 && cols <= cols_pad && ldz >= cols_pad,
         "0 <= rows <= rows_pad, 0 <= cols <= cols_pad <= ldz, rows_pad >= 1, cols_pad >= 1");
    NEED(row0 >= 0 && (long)row0 + rows <= 0x7fffffffL, "row0 >= 0 and row0 + rows <= 2^31 - 1");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_randn_t<T>(ST(stream), seed, stream_id, row0, rows, cols, (T*)Z, ldz, rows_pad, cols_pad);
    });
}

int pg_alpha_batched(pg_handle h, int dtype, int n, const void* Minv, long ldm, long m_stride, const void* y, long y_stride, void* u,
                     long u_stride, void* alpha, long alpha_stride, void* work, long work_stride, int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && y && u && alpha && work, "null pointer");
    NEED(ldm >= n && nexp >= 1 && nexp <= 65535, "bad size");
    NEED16(Minv, ldm); NEEDS16(Minv, m_stride); NEED16(y, y_stride); NEED16(u, u_stride); NEED16(alpha, alpha_stride); NEED16(work, work_stride);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_alpha_batched_t<T>(ST(stream), n, (const T*)Minv, ldm, m_stride, (const T*)y, y_stride, (T*)u, u_stride, (T*)alpha, alpha_stride,
                                     (T*)work, work_stride, nexp);
    });
}

int pg_alpha_nlml_batched(pg_handle h, int dtype, int n_real, int n, const void* Minv, long ldm, long m_stride, const void* y, long y_stride,
                          void* u, long u_stride, void* alpha, long alpha_stride, void* work, long work_stride, double* out, long out_stride,
                          int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && y && u && alpha && work && out, "null pointer");
    NEED(n_real > 0 && n_real <= n && ldm >= n && nexp >= 1 && nexp <= 65535, "bad size");
    NEED16(Minv, ldm); NEEDS16(Minv, m_stride); NEED16(y, y_stride); NEED16(u, u_stride); NEED16(alpha, alpha_stride); NEED16(work, work_stride);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_alpha_batched_t<T>(ST(stream), n, (const T*)Minv, ldm, m_stride, (const T*)y, y_stride, (T*)u, u_stride, (T*)alpha, alpha_stride,
                                     (T*)work, work_stride, nexp, n_real, out, out_stride);
    });
}

int pg_lauum_batched(pg_handle h, int dtype, int n, const void* Minv, long ldm, long m_stride, void* Kinv, long ldk, long k_stride, int nexp,
                     void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && Kinv, "null pointer");
    NEED(Minv != Kinv, "pg_lauum_batched is out of place");
    NEED(nexp >= 1 && nexp <= 65535 && ldm >= n && ldk >= n, "bad size");
    NEED(nexp == 1 || (m_stride >= (long)n * ldm && k_stride >= (long)n * ldk), "experts' matrices overlap");
    NEED16(Minv, ldm); NEEDS16(Minv, m_stride); NEED16(Kinv, ldk); NEEDS16(Kinv, k_stride);
    ExpBatch eb;
    eb.nexp = nexp; eb.eA = k_stride; eb.eInv = 0; eb.eM = m_stride; eb.eX = 0; eb.ehp = 0;
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_lauum_t<T>(h, ST(stream), n, (const T*)Minv, ldm, (T*)Kinv, ldk, &eb);
    });
}

int pg_nlml_grad_batched(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, long hp_stride, const void* X, long ldx, long x_stride,
                         int n, int d, const void* Kinv, long ldk, long k_stride, const void* alpha, long alpha_stride, double* grad,
                         long grad_stride, int nhp, double* work, long lwork, int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && X && Kinv && alpha && grad && work, "null pointer");
    NEED(ldk >= n && ldx >= d, "leading dimension too small");
    NEED16(Kinv, ldk); NEEDS16(Kinv, k_stride);
    if (check_spec(spec, __func__)) return -1;
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_nlml_grad_t<T>(ST(stream), *spec, hp, (const T*)X, ldx, n, d, (const T*)Kinv, ldk, (const T*)alpha, grad, nhp, work, lwork, nexp,
                                 hp_stride, x_stride, k_stride, alpha_stride, grad_stride);
    });
}

int pg_alpha_nlml_async(pg_handle h, int dtype, int n_real, int n, const void* L, long ldl, const void* Minv, long ldm, const void* y,
                        void* u, void* alpha, void* work, double* out, void* stream) {
    JOIN(h, stream);
    NEED(h && L && Minv && y && u && alpha && work && out, "null pointer");
    NEED(n_real > 0 && n_real <= n && ldl >= n && ldm >= n, "bad size");
    NEED16(L, ldl); NEED16(Minv, ldm); NEED16(y, 0); NEED16(u, 0); NEED16(alpha, 0); NEED16(work, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_alpha_nlml_async_t<T>(h, ST(stream), n_real, n, (const T*)L, ldl, (const T*)Minv, ldm, (const T*)y, (T*)u, (T*)alpha, (T*)work, out);
    });
}

int pg_nlml_value(pg_handle h, int dtype, int n, const void* L, long ldl, const void* y, const void* alpha, double* out,
                  void* stream) {
    JOIN(h, stream);
    NEED(h && L && y && alpha && out, "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_nlml_value_t<T>(ST(stream), n, (const T*)L, ldl, (const T*)y, (const T*)alpha, out);
    });
}

long pg_nlml_grad_worksize(int n, int nhp) { return pg_nlml_grad_worksize_impl(n, nhp); }

long pg_kernel_xgrad_worksize(pg_handle h, int m, int n, int d, int nexp) { return h ? pg_xgrad_worksize_impl(h->ncu, m, n, d, nexp) : -1; }

int pg_kernel_xgrad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, long hp_stride, const void* Xq, long ldq, long xq_stride,
                    int m, const void* Z, long ldz, long z_stride, int n, int d, const void* u, long u_stride, void* out_u, long ldou,
                    long ou_stride, const void* B, long ldb, long b_stride, int trans_b, void* out_b, long ldob, long ob_stride, int accumulate,
                    double* work, long lwork, int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && hp && Xq && Z && work, "null pointer");
    NEED(!u == !out_u && !B == !out_b, "u / B need their outputs (and the reverse)");
    NEED(u || B, "neither u nor B given");
    if (check_spec(spec, __func__)) return -1;
    NEED(m >= 0 && n >= 0 && d >= 1 && d <= PG_MAX_DIM, "bad shape (0 <= m, n; 1 <= d <= PG_MAX_DIM)");
    NEED(nexp >= 1 && nexp <= 65535 && (m + 63) / 64 <= 65535, "1 <= nexp <= 65535, m <= 64 * 65535");
    NEED(ldq >= d && ldz >= d, "ldq, ldz >= d");
    NEED(!B || ldb >= (trans_b ? m : n), "ldb too small");
    NEED((!u || ldou >= d) && (!B || ldob >= d), "ldou, ldob >= d");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_xgrad_t<T>(ST(stream), h->ncu, *spec, hp, hp_stride, (const T*)Xq, ldq, xq_stride, m, (const T*)Z, ldz, z_stride, n, d, (const T*)u,
                             u_stride, (T*)out_u, ldou, ou_stride, (const T*)B, ldb, b_stride, trans_b, (T*)out_b, ldob, ob_stride, accumulate, work,
                             lwork, nexp);
    });
}

int pg_nlml_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d,
                 const void* Kinv, long ldk, const void* alpha, double* grad, int nhp, double* work, long lwork,
                 void* stream) {
    JOIN(h, stream);
    NEED(h && hp && X && Kinv && alpha && grad && work, "null pointer");
    NEED(ldk >= n && ldx >= d, "leading dimension too small");
    NEED16(Kinv, ldk);
    if (check_spec(spec, __func__)) return -1;
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_nlml_grad_t<T>(ST(stream), *spec, hp, (const T*)X, ldx, n, d, (const T*)Kinv, ldk, (const T*)alpha, grad, nhp, work, lwork);
    });
}

int pg_predict_mean_q(pg_handle h, int dtype, int n_pad, int m_pad, const void* Ks, long ldks, const void* Minv, long ldm,
                      const void* alpha, void* mean, void* q, double kss, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && Ks && alpha && mean && work, "null pointer");
    NEED(!q || Minv, "variance needs Minv");
    NEED(ldks >= m_pad && (!Minv || ldm >= n_pad), "bad leading dimension");
    NEED16(Ks, ldks); NEED16(Minv, ldm); NEED16(alpha, 0); NEED16(work, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_predict_mean_q_t<T>(h, ST(stream), n_pad, m_pad, (const T*)Ks, ldks, (const T*)Minv, ldm, (const T*)alpha, (T*)mean, (T*)q, kss,
                                      (T*)work);
    });
}

int pg_predict_mean_q_kt(pg_handle h, int dtype, int n_pad, int m_pad, const void* Kt, long ldkt, const void* Minv, long ldm,
                         const void* alpha, void* mean, void* q, double kss, void* work, void* stream) {
    JOIN(h, stream);
    NEED(h && Kt && alpha && mean && work, "null pointer");
    NEED(!q || Minv, "variance needs Minv");
    NEED(ldkt >= n_pad && (!Minv || ldm >= n_pad), "bad leading dimension");
    NEED16(Kt, ldkt); NEED16(Minv, ldm); NEED16(alpha, 0); NEED16(work, 0);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_predict_mean_q_kt_t<T>(h, ST(stream), n_pad, m_pad, (const T*)Kt, ldkt, (const T*)Minv, ldm, (const T*)alpha, (T*)mean, (T*)q, kss,
                                         (T*)work);
    });
}

int pg_predict_mean_q_kt_batched(pg_handle h, int dtype, int n_pad, int m_pad, const void* Kt, long ldkt, long kt_stride, const void* Minv,
                                 long ldm, long m_stride, const void* alpha, long alpha_stride, void* mean, long mean_stride, void* var,
                                 long var_stride, const pg_covspec* spec, const double* hp, long hp_stride, void* work, long work_stride,
                                 int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && Kt && alpha && mean && work, "null pointer");
    NEED(!var || (Minv && hp), "variance needs Minv and hp");
    if (var && check_spec(spec, __func__)) return -1;
    NEED(nexp >= 1 && nexp <= 65535, "1 <= nexp <= 65535");
    NEED(ldkt >= n_pad && (!Minv || ldm >= n_pad), "bad leading dimension");
    NEED16(Kt, ldkt); NEEDS16(Kt, kt_stride); NEED16(Minv, ldm); NEEDS16(Minv, m_stride); NEED16(alpha, alpha_stride); NEED16(work, work_stride);
    NEED(nexp == 1 || (mean_stride >= m_pad && (!var || (var_stride >= m_pad && work_stride >= (long)(n_pad / 64) * m_pad))),
         "experts' outputs / workspaces overlap");
    static const pg_covspec none = {};
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_predict_mean_q_kt_batched_t<T>(h, ST(stream), n_pad, m_pad, (const T*)Kt, ldkt, kt_stride, (const T*)Minv, ldm, m_stride,
                                                 (const T*)alpha, alpha_stride, (T*)mean, mean_stride, (T*)var, var_stride, spec ? *spec : none, hp,
                                                 hp_stride, (T*)work, work_stride, nexp);
    });
}

int pg_trmm_lower(pg_handle h, int dtype, int n_pad, int m_pad, const void* Minv, long ldm, const void* Ks, long ldks,
                  void* V, long ldv, void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && Ks && V, "null pointer");
    NEED(ldm >= n_pad && ldks >= m_pad && ldv >= m_pad, "bad leading dimension");
    NEED16(Minv, ldm); NEED16(Ks, ldks); NEED16(V, ldv);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_trmm_lower_t<T>(h, ST(stream), n_pad, m_pad, (const T*)Minv, ldm, (const T*)Ks, ldks, (T*)V, ldv);
    });
}

int pg_syrk_tn_sub(pg_handle h, int dtype, int m_pad, int n_pad, const void* V, long ldv, void* C, long ldc, int lower_only,
                   void* stream) {
    JOIN(h, stream);
    NEED(h && V && C, "null pointer");
    NEED(ldv >= m_pad && ldc >= m_pad, "bad leading dimension");
    NEED16(V, ldv); NEED16(C, ldc);
    AtomicGuard ag(h, C);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_syrk_tn_sub_t<T>(h, ST(stream), m_pad, n_pad, (const T*)V, ldv, (T*)C, ldc, lower_only);
    });
}

int pg_trmm_lower_kt_batched(pg_handle h, int dtype, int n_pad, int m_pad, const void* Minv, long ldm, long m_stride, const void* Kt, long ldkt,
                             long kt_stride, void* Vt, long ldvt, long vt_stride, int nexp, void* stream) {
    JOIN(h, stream);
    NEED(h && Minv && Kt && Vt, "null pointer");
    NEED(nexp >= 1 && nexp <= 65535, "1 <= nexp <= 65535");
    NEED(ldm >= n_pad && ldkt >= n_pad && ldvt >= n_pad && Kt != Vt, "bad leading dimension / aliasing");
    NEED(nexp == 1 || vt_stride >= (long)m_pad * ldvt, "experts' outputs overlap");
    NEED16(Minv, ldm); NEEDS16(Minv, m_stride); NEED16(Kt, ldkt); NEEDS16(Kt, kt_stride); NEED16(Vt, ldvt); NEEDS16(Vt, vt_stride);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_trmm_lower_kt_t<T>(h, ST(stream), n_pad, m_pad, (const T*)Minv, ldm, m_stride, (const T*)Kt, ldkt, kt_stride, (T*)Vt, ldvt, vt_stride,
                                     nexp);
    });
}

int pg_syrk_nt_sub_batched(pg_handle h, int dtype, int m_pad, int n_pad, const void* Vt, long ldvt, long vt_stride, void* C, long ldc,
                           long c_stride, int nexp, int lower_only, void* stream) {
    JOIN(h, stream);
    NEED(h && Vt && C, "null pointer");
    NEED(nexp >= 1 && nexp <= 65535, "1 <= nexp <= 65535");
    NEED(ldvt >= n_pad && ldc >= m_pad, "bad leading dimension");
    NEED(nexp == 1 || (vt_stride >= (long)m_pad * ldvt && c_stride >= (long)m_pad * ldc), "experts' matrices overlap");
    NEED16(Vt, ldvt); NEEDS16(Vt, vt_stride); NEED16(C, ldc); NEEDS16(C, c_stride);
    AtomicGuard ag(h, C);
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_syrk_nt_sub_t<T>(h, ST(stream), m_pad, n_pad, (const T*)Vt, ldvt, vt_stride, (T*)C, ldc, c_stride, nexp, lower_only);
    });
}

int pg_grbcm_local_terms(pg_handle h, int dtype, int m, const void* mean_c, const void* var_c, const void* var_g,
                         int is_first, int accumulate, double* out, long ldo, double* beta_out, double* prec_out,
                         void* stream) {
    JOIN(h, stream);
    NEED(h && mean_c && var_c && var_g && out, "null pointer");
    NEED(ldo >= m, "ldo < m");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_grbcm_terms_t<T>(ST(stream), m, (const T*)mean_c, (const T*)var_c, (const T*)var_g, is_first, accumulate, out, ldo, beta_out, prec_out);
    });
}

int pg_grbcm_local_terms_batched(pg_handle h, int dtype, int m, const void* mean_l, long mean_stride, const void* var_l, long var_stride,
                                 const void* var_g, int nexp, int first, int accumulate, double* out, long ldo, double* beta_out,
                                 double* prec_out, long ldb, void* stream) {
    JOIN(h, stream);
    NEED(h && mean_l && var_l && var_g && out, "null pointer");
    NEED(ldo >= m && nexp >= 1 && (nexp == 1 || (!beta_out && !prec_out) || ldb >= m), "bad size");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_grbcm_terms_batched_t<T>(ST(stream), m, (const T*)mean_l, mean_stride, (const T*)var_l, var_stride, (const T*)var_g, nexp, first,
                                           accumulate, out, ldo, beta_out, prec_out, ldb);
    });
}

int pg_grbcm_finish(pg_handle h, int dtype, int m, const double* sums, long lds, const void* mean_g, const void* var_g,
                    void* mean, void* var, double* beta0, double* prec0, void* stream) {
    JOIN(h, stream);
    NEED(h && sums && mean_g && var_g && mean && var, "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_grbcm_finish_t<T>(ST(stream), m, sums, lds, (const T*)mean_g, (const T*)var_g, (T*)mean, (T*)var, beta0, prec0);
    });
}

int pg_grbcm_weighted_prec(pg_handle h, int dtype, int m, int m_pad, const void* P, long ldp, const double* beta, void* acc,
                           long lda, int accumulate, void* stream) {
    JOIN(h, stream);
    NEED(h && P && beta && acc, "null pointer");
    NEED(m_pad >= m && ldp >= m && lda >= m_pad, "inconsistent sizes");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_weighted_prec_t<T>(ST(stream), m, m_pad, (const T*)P, ldp, beta, (T*)acc, lda, accumulate);
    });
}

int pg_symmetrize(pg_handle h, int dtype, int n, void* A, long lda, void* stream) {
    JOIN(h, stream);
    NEED(h && A, "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_symmetrize_t<T>(ST(stream), n, (T*)A, lda);
    });
}

int pg_grbcm_finish_full(pg_handle h, int dtype, int m, const double* sums, long lds, const void* mean_g, const void* var_g,
                         const void* cov, long ldc, void* mean, void* stream) {
    JOIN(h, stream);
    NEED(h && sums && mean_g && var_g && cov && mean, "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_grbcm_finish_full_t<T>(ST(stream), m, sums, lds, (const T*)mean_g, (const T*)var_g, (const T*)cov, ldc, (T*)mean);
    });
}

int pg_sqdist_argmin(pg_handle h, int dtype, const void* X, long ldx, int n, const void* C, long ldc, int m, int d, void* D,
                     long ldd, int* idx, void* stream) {
    JOIN(h, stream);
    NEED(h && X && C && (D || idx), "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_centres<T>(ST(stream), (const T*)X, ldx, n, (const T*)C, ldc, m, d, (T*)D, ldd, idx);
    });
}

int pg_tril(pg_handle h, int dtype, int n, void* A, long lda, void* stream) {
    JOIN(h, stream);
    NEED(h && A, "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_tril_t<T>(ST(stream), n, (T*)A, lda);
    });
}

int pg_set_lookahead(pg_handle h, int on) {
    NEED(h, "null handle");
    h->lookahead = (on && h->upd) ? 1 : 0;
    return 0;
}

int pg_set_outer_panel(pg_handle h, int columns) {
    NEED(h, "null handle");
    NEED(columns == 0 || (columns >= 128 && columns % 128 == 0 && columns <= 2048), "outer panel must be 0 (automatic) or a multiple of 128 up to 2048");
    h->nbo = columns;
    return 0;
}

int pg_set_recursive_split(pg_handle h, int min_n) {
    NEED(h, "null handle");
    NEED(min_n == 0 || (min_n >= 512 && min_n % 512 == 0), "min_n must be 0 (never) or a multiple of 512");
    h->rec_min = min_n;
    return 0;
}

int pg_profile(pg_handle h, int on) {
    NEED(h, "null handle");
    if (on) { h->prof_flops = 0; h->prof_ms = 0; h->prof_launches = 0; }
    h->prof_on = on;
    return 0;
}
int pg_set_coupled_chain(pg_handle h, int on) {
    NEED(h, "null handle");
    if (on < 0) {       // off for now, as after a time-out: the rows stream stays and the handle re-arms itself (pg_set_rearm_after)
        if (h->coupled || h->tmo_off == 0) { h->tmo_off = h->rows ? 1 : 0; h->calls_since_tmo = 0; }
        h->coupled = 0;
        return 0;
    }
    h->tmo_off = 0;
    h->rearm_cur = h->rearm_after;
    h->rearms_seen = h->rearms;      // an explicit switch forgets the back-off's history: the next time-out starts from rearm_after again
    h->calls_since_rearm = 0;
    if (!on) {
        // off also RELEASES the rows stream (the handle then owns two streams)
        if (h->rows) {
            PG_CHECK(hipStreamSynchronize(h->rows));
            PG_CHECK(hipStreamDestroy(h->rows));
            h->rows = nullptr;
        }
        h->coupled = 0;
        return 0;
    }
    if (!h->rows && h->upd) {
        int prio_lo = 0, prio_hi = 0;
        PG_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        if (hipStreamCreateWithPriority(&h->rows, hipStreamNonBlocking, prio_hi) != hipSuccess) {
            h->rows = nullptr;
            (void)hipGetLastError();
        }
    }
    h->coupled = (h->rows && probe_concurrent_queues(h)) ? 1 : 0;
    return 0;
}
int pg_coupled_chain(pg_handle h) { return h ? h->coupled : -1; }
int pg_last_coupled_panels(pg_handle h) {
    if (!h) return -1;
    return h->last_coupled;
}
int pg_profile_read(pg_handle h, double* flops, double* ms, long* launches) {
    NEED(h, "null handle");
    if (flops) *flops = h->prof_flops;
    if (ms) *ms = h->prof_ms;
    if (launches) *launches = h->prof_launches;
    return 0;
}

int pg_set_spin_budget(pg_handle h, long microseconds) {
    NEED(h, "null handle");
    h->spin_ticks = microseconds < 0 ? -1 : (long long)microseconds * 100;      // 0: scaled to the call
    return 0;
}
int pg_set_rearm_after(pg_handle h, int calls) {
    NEED(h, "null handle");
    NEED(calls >= 0, "calls must be >= 0 (0: never re-arm automatically)");
    h->rearm_after = calls;
    h->rearm_cur = calls;
    h->rearms_seen = h->rearms;
    h->calls_since_rearm = 0;
    return 0;
}
int pg_chain_rearms(pg_handle h) { return h ? h->rearms : -1; }
long pg_wait_budget_us(pg_handle h, int n) {
    if (!h) return 0;
    const long long t = pg_wait_ticks(h, n);
    return t < 0 ? -1 : (long)(t / 100);
}
// scratch: 4 ints + 2 long longs of device memory (32 bytes, 8-byte aligned).  The handle's state is not touched (no pinned word, no
// switch to the classic chain): the probe only measures the wait.
int pg_spin_probe(pg_handle h, int n, void* scratch, void* stream) {
    NEED(h && scratch, "null pointer");
    PG_CHECK(hipMemsetAsync(scratch, 0, 32, ST(stream)));
    int* w = reinterpret_cast<int*>(scratch);
    const CsWait cw = {w + 1, nullptr, pg_wait_ticks(h, n), 1};
    return pg_spin_probe_launch(ST(stream), w, cw, reinterpret_cast<long long*>(w + 4));
}
int pg_chain_timeouts(pg_handle h) {
    if (!h) return -1;
    poll_timeout(h);
    return h->timeouts;
}

// Blocking form of pg_build_potrf_trtri: waits for the factorisation and, when a wait of the coupled chain expired (info = -1),
// repeats the whole call -- covariance build included, the first attempt's A is garbage -- on the classic chain before it returns.
int pg_build_potrf_trtri_checked(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n,
                                 int d, double jitter, void* A, long lda, int n_pad, void* inv_diag, int* info, void* Minv, long ldm,
                                 void* stream, int* info_host) {
    NEED(info_host, "null pointer");
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int rc = pg_build_potrf_trtri(h, dtype, spec, hp, X, ldx, n, d, jitter, A, lda, n_pad, inv_diag, info, Minv, ldm, stream);
        if (rc) return rc;
        PG_CHECK(hipMemcpyAsync(info_host, info, sizeof(int), hipMemcpyDeviceToHost, ST(stream)));
        PG_CHECK(hipStreamSynchronize(ST(stream)));
        if (*info_host >= 0) return 0;
        poll_timeout(h);
        if (h->coupled) { h->tmo_off = 1; h->calls_since_tmo = 0; }
        h->coupled = 0;        // whatever the pinned word said: the repeat must not take the coupled chain
    }
    return 0;
}

int pg_leaf_raw(pg_handle h, int dtype, void* A, long lda, void* inv, long ldi, int* info, void* stream) {
    JOIN(h, stream);
    NEED(h && A && info, "null pointer");
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_leaf<T>(ST(stream), (T*)A, lda, (T*)inv, ldi, info, 0);
    });
}

int pg_rowstep_raw(pg_handle h, int dtype, int n, void* A, long lda, int o0, int k0, const void* inv, int* flags, int* info, void* stream) {
    JOIN(h, stream);
    NEED(h && A && inv && flags && info, "null pointer");
    NEED(n % 128 == 0 && k0 % 128 == 0 && o0 % 128 == 0 && o0 <= k0 && k0 + 128 < n, "bad shape");
    // every flag the kernel waits for is already up (64 >= any count): the kernel alone, nothing to wait for
    PG_CHECK(hipMemsetAsync(flags, 0x40, 8 * sizeof(int), ST(stream)));
    PG_CHECK(hipMemsetAsync(flags + 6, 0, 2 * sizeof(int), ST(stream)));   // [6]: time-out word, [7]: spare
    const CsWait cw = {flags + 6, nullptr, 200000000LL, 1};
    return dispatch(dtype, __func__, [&](auto t) { using T = decltype(t);
        return pg_rowstep<T>(ST(stream), (T*)A, lda, n, o0, k0, 1, (const T*)inv, flags, flags + 1, flags + 2, cw, info, flags + 3, flags + 4, 0);
    });
}

int pg_gemm_raw(pg_handle h, int dtype, int variant, int M, int N, int K, double alpha, const void* A, long lda,
                const void* B, long ldb, double beta, void* C, long ldc, int tri, int klo, int khi, void* stream) {
    JOIN(h, stream);
    NEED(h && A && B && C, "null pointer");
    NEED(variant == GEMM_NT_128 || variant == GEMM_NT_RP || variant == GEMM_NN_128 || variant == GEMM_TN_128 ||
             variant == GEMM_TT_128 || variant == GEMM_NT_64 || variant == GEMM_NT_64x128 || variant == GEMM_NT_32x64 ||
             variant == GEMM_NT_32x128 || variant == GEMM_TT_64 || variant == GEMM_NT_32x32 || variant == GEMM_TN_64 ||
             variant == GEMM_NT_128_PL || variant == GEMM_NN_128_PL || variant == GEMM_TN_128_PL || variant == GEMM_TT_128_PL,
         "variant not exposed");
    NEED16(A, lda); NEED16(B, ldb); NEED16(C, ldc);
    AtomicGuard ag(h, C);
    return dispatch(dtype, __func__, [&](auto t) {
        return gemm_raw_t<decltype(t)>(h, variant, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, tri, klo, khi, stream);
    });
}

// ---- the nearest-neighbour (Vecchia) GP (include/pygpr_hip_vecchia.h)
int pg_knn(pg_handle h, int dtype, const void* Xq, long ldq, int q, const void* Xc, long ldc, int n, int d, const double* s, int m, int causal,
           int* nbr, long ldn, void* stream) {
    JOIN(h, stream);
    NEED(dtype == PG_F64, "float64 only (dtype must be PG_F64)");
    if (!(q >= 0 && n >= 0 && d >= 1 && d <= PG_MAX_DIM && m >= 1 && m <= 63)) {
        pg_set_error("%s: bad shape (0 <= q, n; 1 <= d <= PG_MAX_DIM; 1 <= m <= 63)", __func__);
        return -2;
    }
    NEED(ldq >= d && ldc >= d && ldn >= m, "ldq, ldc >= d and ldn >= m");
    NEED(!causal || q <= n, "a causal search takes its queries from the candidates (q <= n)");
    NEED(h, "null handle");
    if (q == 0) return 0;
    NEED(Xq && nbr && (Xc || n == 0), "null pointer");
    return pg_knn_impl(ST(stream), (const double*)Xq, ldq, q, (const double*)Xc, ldc, n, d, s, m, causal, nbr, ldn);
}

// what pg_vecchia_nlml_grad and pg_vecchia_predict ask of their common arguments; nhp < 0: the offsets are not held to an extent
static int check_vecchia(const char* fn, pg_handle h, int dtype, const pg_covspec* spec, const double* hp, int nhp, int n, int d, int m, long ldx,
                         long ldn) {
    if (!spec) { pg_set_error("%s: null covariance spec", fn); return -1; }
    if (dtype != PG_F64) { pg_set_error("%s: float64 only (dtype must be PG_F64)", fn); return -1; }
    if (check_spec(spec, fn)) return -1;      // (PG_KIND_SQDIST is refused: it is no covariance)
    if (!(n >= 0 && d >= 1 && d <= PG_MAX_DIM && m >= 1 && m <= 63)) {
        pg_set_error("%s: bad shape (0 <= n; 1 <= d <= PG_MAX_DIM; 1 <= m <= 63)", fn);
        return -2;
    }
    for (int c = 0; c < (spec->ncomp & ~PG_SPEC_PRODUCT); ++c) {
        const int w = spec->kind[c] == PG_KIND_PERIODIC ? 2 * d + 1 : (spec->kind[c] == PG_KIND_RQ ? d + 2 : d + 1);
        if (spec->off[c] < 0 || (nhp >= 0 && spec->off[c] + w > nhp)) { pg_set_error("%s: a component's block lies outside hp", fn); return -1; }
    }
    for (int c = 0; c < spec->nnoise; ++c)
        if (spec->noise_off[c] < 0 || (nhp >= 0 && spec->noise_off[c] >= nhp)) { pg_set_error("%s: a noise entry lies outside hp", fn); return -1; }
    if (ldx < d || ldn < m) { pg_set_error("%s: ldx >= d and ldn >= m", fn); return -1; }
    if (!h || !hp) { pg_set_error("%s: null handle or hp", fn); return -1; }      // (last: the refusals above need no device)
    return 0;
}

long pg_vecchia_nlml_grad_worksize(int count, int d, int nhp) {
    return (count >= 0 && d >= 1 && d <= PG_MAX_DIM && nhp >= 0) ? pg_vecchia_worksize_impl(count, d, nhp) : -1;
}

int pg_vecchia_nlml_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, int nhp, const void* X, long ldx, int n, int d,
                         const void* Y, const int* nbr, long ldn, int m, int first, int count, double jitter, int want_grad, void* cmean,
                         void* cvar, double* out, double* grad, int* info, void* work, void* stream) {
    JOIN(h, stream);
    NEED(nhp >= 0, "negative nhp");
    NEED(n < 0 || (first >= 0 && count >= 0 && (long)first + count <= n), "0 <= first, count and first + count <= n");
    if (int rc = check_vecchia(__func__, h, dtype, spec, hp, nhp, n, d, m, ldx, ldn)) return rc;
    NEED(out && info && (work || count == 0) && (grad || !want_grad), "null pointer");
    NEED(count == 0 || (X && Y && nbr && cmean && cvar), "null pointer");
    return pg_vecchia_nlml_grad_impl(ST(stream), *spec, hp, nhp, (const double*)X, ldx, n, d, (const double*)Y, nbr, ldn, m, first, count, jitter,
                                     want_grad, (double*)cmean, (double*)cvar, out, grad, info, (double*)work);
}

long pg_vecchia_predict_worksize(int q, int d) { return (q >= 0 && d >= 1 && d <= PG_MAX_DIM) ? pg_vecchia_worksize_impl(q, d, 0) : -1; }

int pg_vecchia_predict(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d, const void* Y,
                       const void* Xq, long ldq, int q, const int* nbr, long ldn, int m, double jitter, void* mean, void* var, int* info,
                       void* work, void* stream) {
    JOIN(h, stream);
    NEED(q >= 0 && ldq >= d, "q >= 0 and ldq >= d");
    if (int rc = check_vecchia(__func__, h, dtype, spec, hp, -1, n, d, m, ldx, ldn)) return rc;
    NEED(info && (work || q == 0), "null pointer");
    NEED(q == 0 || (Xq && nbr && mean && (n == 0 || (X && Y))), "null pointer");
    return pg_vecchia_predict_impl(ST(stream), *spec, hp, (const double*)X, ldx, n, d, (const double*)Y, (const double*)Xq, ldq, q, nbr, ldn, m,
                                   jitter, (double*)mean, (double*)var, info, (double*)work);
}

}  // extern "C"
