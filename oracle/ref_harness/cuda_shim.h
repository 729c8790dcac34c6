/*
 * cuda_shim.h -- the CUDA surface the reference's subsweep.h and shiftCells.h use, supplied for a
 * host compiler so that their device functions run on the CPU unchanged (TEST INFRASTRUCTURE ONLY).
 *
 * The reference's text is never copied: ref_main.cpp #include's it from the reference tree at build
 * time, after this header.  What the reference leaves to the CUDA toolchain is decided here:
 *
 *   threads      threadIdx / blockIdx are thread_local, blockDim / gridDim plain; __syncthreads is a
 *                real barrier while shiftCells runs (one OS thread per cell) and a no-op while
 *                subsweep_kernel runs (its threads run one after another, ref_main.cpp says why);
 *   __shared__   static storage: one array for the one block;
 *   random       no cuRAND.  The draws are the project's own (include/pmc_detmath.h), keyed by the
 *                cell the harness is executing, the sweep and the seed; curand_init's arguments are
 *                ignored.  Of a cell visit the reference draws, in this order,
 *                    atom_counts uniforms    (random_shuffle -> random_int: (int)u % (i + 1));
 *                    per move m: 3 normals   (make_move), then at most one uniform (accept_move).
 *                ref_rng_* REQUIRE exactly that pattern and abort on anything else, so the draw
 *                structure the oracle assumes is checked on every visit.
 *                  shuffle uniform   0.5: any u < 1 gives (int)u == 0, as cuRAND's (0, 1] does for
 *                                    all but u == 1 (quirk R1);
 *                  normal 3m + dim   component dim of pmc_move_normals of PMC_TAG_MOVE call m;
 *                  uniform of move m exp(-T), T = pmc_accept_threshold of PMC_TAG_ACCEPT call m, so
 *                                    that u < exp(-beta dE) is the oracle's beta dE < T.
 *                curand_uniform and __expf return double: the comparison then differs from the
 *                oracle's only by exp's rounding (1e-16), and what remains between the two is the
 *                energy arithmetic itself.
 *   __powf       pow in double, rounded to float (CUDA's is an approximation of that).
 *
 * Needs <cmath>, <cstdio>, <cstdlib>, <cstdint>, <pthread.h> and pmc_detmath.h included before it.
 */
#ifndef REF_CUDA_SHIM_H
#define REF_CUDA_SHIM_H

#define __device__
#define __global__
#define __shared__ static

struct ref_dim3 { int x, y, z; };
static thread_local ref_dim3 threadIdx, blockIdx;
static ref_dim3 blockDim, gridDim;

static pthread_barrier_t ref_barrier;
static bool ref_barrier_on = false;
#define __syncthreads() ref_syncthreads()
static inline void ref_syncthreads() {
    if (ref_barrier_on) pthread_barrier_wait(&ref_barrier);
}

#define __powf(x, y) ref_powf((x), (y))
#define __expf(x) ref_expf((x))
static inline float ref_powf(float x, float y) { return (float)pow((double)x, (double)y); }
static inline double ref_expf(double x) { return exp(x); }

/* ---- random numbers ------------------------------------------------------------------------- */
struct curandState_t { int unused; };

struct ref_rng_t {
    uint32_t cell, sweep, k0, k1;
    int shuffle_left;      /* shuffle uniforms still expected */
    int normals;           /* normals drawn so far in this visit */
    bool uniform_drawn;    /* the current move's uniform was drawn */
    float g[3];            /* the current move's normals */
};
static ref_rng_t ref_rng;

#define REF_REQUIRE(cond, what)                                                                   \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            fprintf(stderr, "ref_harness: draw pattern violated: %s (cell %u, %d normals so far)\n", \
                    what, ref_rng.cell, ref_rng.normals);                                         \
            abort();                                                                              \
        }                                                                                         \
    } while (0)

/* before a thread of subsweep_kernel runs: the cell it will visit and that cell's count */
static inline void ref_rng_begin(uint32_t cell, int atom_counts, uint32_t sweep, uint64_t seed) {
    ref_rng.cell = cell;
    ref_rng.sweep = sweep;
    ref_rng.k0 = (uint32_t)seed;
    ref_rng.k1 = (uint32_t)(seed >> 32);
    ref_rng.shuffle_left = atom_counts;
    ref_rng.normals = 0;
    ref_rng.uniform_drawn = false;
}

/* after it: every shuffle uniform was drawn, and 3 normals for each of `moves` moves (none at all
 * for an empty cell) */
static inline void ref_rng_end(int atom_counts, int moves) {
    REF_REQUIRE(ref_rng.shuffle_left == 0, "shuffle uniforms left over");
    REF_REQUIRE(ref_rng.normals == (atom_counts > 0 ? 3 * moves : 0), "normals drawn != 3 * n_M");
}

template <class... A>
static inline void curand_init(A...) {}

static inline double curand_uniform(curandState_t*) {
    if (ref_rng.shuffle_left > 0) {
        --ref_rng.shuffle_left;
        return 0.5;
    }
    REF_REQUIRE(ref_rng.normals > 0 && ref_rng.normals % 3 == 0, "uniform outside a finished group of 3 normals");
    REF_REQUIRE(!ref_rng.uniform_drawn, "second uniform in one move");
    ref_rng.uniform_drawn = true;
    const uint32_t m = (uint32_t)(ref_rng.normals / 3 - 1);
    const float T = pmc_accept_threshold(
        pmc_philox4x32_10(m, ref_rng.cell, ref_rng.sweep, PMC_TAG_ACCEPT, ref_rng.k0, ref_rng.k1));
    return exp(-(double)T);
}

static inline float curand_normal(curandState_t*) {
    REF_REQUIRE(ref_rng.shuffle_left == 0, "normal before the shuffle's uniforms were all drawn");
    const int dim = ref_rng.normals % 3;
    if (dim == 0) {
        const uint32_t m = (uint32_t)(ref_rng.normals / 3);
        pmc_move_normals(pmc_philox4x32_10(m, ref_rng.cell, ref_rng.sweep, PMC_TAG_MOVE, ref_rng.k0, ref_rng.k1),
                         &ref_rng.g[0], &ref_rng.g[1], &ref_rng.g[2]);
        ref_rng.uniform_drawn = false;
    }
    ++ref_rng.normals;
    return ref_rng.g[dim];
}

#endif /* REF_CUDA_SHIM_H */
