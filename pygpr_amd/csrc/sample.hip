// Standard normal variates from a counter-based generator (include/pygpr_hip_sample.h): Philox4x32-10 keyed by the seed, counter
// (column pair, row, stream, 0), two 53-bit uniforms per block and a Box-Muller transform in fp64, so that element (row, q) depends on
// (seed, stream, row, q) alone.  A thread produces one 16-byte word of the output -- one block in fp64, two in fp32 -- and consecutive
// lanes consecutive words of a row (a wavefront stores 1 KiB per instruction); no LDS, no atomics, no state between workgroups.
// The work per block is the ten rounds (two 32 x 32 -> 64 bit products each) and one fp64 log, sqrt and sincos.
#include "linalg.h"

#define LAUNCH_CHECK() PG_CHECK(hipGetLastError())

typedef double pg_d2 __attribute__((ext_vector_type(2)));
template <typename T> struct RnVec;
template <> struct RnVec<double> { typedef pg_d2 type; };
template <> struct RnVec<float> { typedef pg_f4 type; };

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

// The two normals of block (j, row, stream): even column in z0, odd column in z1.
__device__ __forceinline__ void philox_normal_pair(unsigned k0, unsigned k1, unsigned j, unsigned row, unsigned stream, double& z0, double& z1) {
    unsigned c0 = j, c1 = row, c2 = stream, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
        const unsigned h0 = __umulhi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
        const unsigned h1 = __umulhi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    }
    const unsigned long long a = ((unsigned long long)(c0 >> 5) << 26) | (unsigned long long)(c1 >> 6);
    const unsigned long long b = ((unsigned long long)(c2 >> 5) << 26) | (unsigned long long)(c3 >> 6);
    const double u1 = (double)(a + 1ull) * 0x1p-53;      // (0, 1]: at most 2^53, exact
    const double u2 = (double)b * 0x1p-53;               // [0, 1), exact
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(6.283185307179586476925 * u2, &s, &c);
    z0 = rad * c;
    z1 = rad * s;
}

// Word t of the launch is word t % wpr of row t / wpr (wpr = ceil(cols_pad / V) words per row); the word's V elements are normals
// where r < rows and q < cols and zero elsewhere.  vec: Z and ldz keep every full word 16-byte aligned.
template <typename T>
__global__ __launch_bounds__(256) void randn_kernel(unsigned k0, unsigned k1, unsigned stream, unsigned row0, int rows, int cols, T* __restrict__ Z,
                                                    long ldz, int rows_pad, int cols_pad, int wpr, int vec) {
    typedef typename RnVec<T>::type vec_t;
    constexpr int V = 16 / (int)sizeof(T);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)rows_pad * wpr) return;
    const int r = (int)(t / wpr), q0 = (int)(t % wpr) * V;
    T v[V];
#pragma unroll
    for (int b = 0; b < V / 2; ++b) {
        double z0 = 0.0, z1 = 0.0;
        const int q = q0 + 2 * b;
        if (r < rows && q < cols) philox_normal_pair(k0, k1, (unsigned)q >> 1, row0 + (unsigned)r, stream, z0, z1);
        v[2 * b] = (T)z0;
        v[2 * b + 1] = (q + 1 < cols) ? (T)z1 : (T)0;      // an odd cols uses half of its last block
    }
    T* dst = Z + (long)r * ldz + q0;
    if (vec && q0 + V <= cols_pad) {
        vec_t w;
#pragma unroll
        for (int e = 0; e < V; ++e) w[e] = v[e];
        *reinterpret_cast<vec_t*>(dst) = w;
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (q0 + e < cols_pad) dst[e] = v[e];
    }
}

template <typename T>
int pg_randn_t(hipStream_t st, long seed, int stream_id, int row0, int rows, int cols, T* Z, long ldz, int rows_pad, int cols_pad) {
    constexpr int V = 16 / (int)sizeof(T);
    const int wpr = (cols_pad + V - 1) / V;
    const long blocks = ((long)rows_pad * wpr + 255) / 256;
    if (blocks > 0x7fffffffL) { pg_set_error("pg_randn: %d x %d is more than one launch covers", rows_pad, cols_pad); return -2; }
    const unsigned long long s = (unsigned long long)seed;
    const int vec = reinterpret_cast<uintptr_t>(Z) % 16 == 0 && (ldz * (long)sizeof(T)) % 16 == 0;
    hipLaunchKernelGGL(randn_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (unsigned)(s & 0xffffffffull), (unsigned)(s >> 32), (unsigned)stream_id,
                       (unsigned)row0, rows, cols, Z, ldz, rows_pad, cols_pad, wpr, vec);
    LAUNCH_CHECK();
    return 0;
}

#define INST(T) template int pg_randn_t<T>(hipStream_t, long, int, int, int, int, T*, long, int, int);
INST(double)
INST(float)
