/*
 * ref_main.cpp -- host harness around the reference's own subsweep.h and shiftCells.h
 * (TEST INFRASTRUCTURE ONLY; built into oracle/_ref/, never committed as a binary).
 *
 * The reference takes its configuration as macros, so one binary is one configuration: the Makefile
 * passes REF_CPS, REF_W, REF_NMAX, REF_NM, REF_SIGMA and REF_BETA, and the include path chooses the
 * root copy of shiftCells.h or the Visual Studio copy.  cuda_shim.h supplies the CUDA surface and
 * the project's random numbers.
 *
 *   ref_X info                              the configuration, one line
 *   ref_X phase IN OUT ox oy oz sweep seed  one colour phase: subsweep_kernel, offset (ox, oy, oz)
 *   ref_X shift IN OUT f dbits              one shiftCells along axis f by the float with bits dbits (hex)
 *
 * A state file is disk (float32[cells * 3 * nmax], the reference layout) followed by n
 * (int16[cells]), little endian.  On output the slots at or past a cell's count are unspecified:
 * shiftCells copies its whole local array, initialised or not, back to disk.
 *
 * Execution model, from the reference's code:
 *   subsweep_kernel  returns early for an empty cell, before a __syncthreads, and its threads share
 *                    nothing but disjoint ranges of D_sh; cells of one colour are never neighbours,
 *                    so no thread reads what another writes.  Its threads run one after another
 *                    here, __syncthreads a no-op.
 *   shiftCells       updates disk and n in place and relies on its barriers (every thread reads its
 *                    neighbour's row before any thread writes).  One OS thread per cell, a real
 *                    barrier.  It overruns its local array when a cell would exceed nmax, so the new
 *                    counts are computed first (new_counts_fit) and such inputs are refused.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <pthread.h>
#include <thread>
#include <vector>

#include "../../include/pmc_detmath.h"
#include "cuda_shim.h"

#if !defined(REF_CPS) || !defined(REF_W) || !defined(REF_NMAX) || !defined(REF_NM) || !defined(REF_SIGMA) || \
    !defined(REF_BETA)
#error "pass -DREF_CPS -DREF_W -DREF_NMAX -DREF_NM -DREF_SIGMA -DREF_BETA (see the Makefile)"
#endif
static_assert(REF_CPS >= 4 && REF_CPS % 2 == 0, "even boxes of at least 4 cells per side");

/* the reference's two kernels (defined at the end of this file by the #include's) */
void subsweep_kernel(float* disk, short int* n, int* offset);
void shiftCells(float* disk, short int* n, int f, float d);

static const int kCps = REF_CPS, kNmax = REF_NMAX, kMoves = REF_NM;
static const int kCells = REF_CPS * REF_CPS * REF_CPS;
static const float kW = REF_W;

static int fail(const char* what) {
    fprintf(stderr, "ref_harness: %s\n", what);
    return 2;
}

static bool read_state(const char* path, std::vector<float>& disk, std::vector<short>& n) {
    disk.assign((size_t)kCells * 3 * kNmax, 0.0f);
    n.assign((size_t)kCells, 0);
    FILE* fp = fopen(path, "rb");
    if (!fp) return false;
    bool ok = fread(disk.data(), sizeof(float), disk.size(), fp) == disk.size() &&
              fread(n.data(), sizeof(short), n.size(), fp) == n.size() && fgetc(fp) == EOF;
    fclose(fp);
    for (int c = 0; ok && c < kCells; ++c) ok = n[c] >= 0 && n[c] <= kNmax;
    return ok;
}

static bool write_state(const char* path, const std::vector<float>& disk, const std::vector<short>& n) {
    FILE* fp = fopen(path, "wb");
    if (!fp) return false;
    bool ok = fwrite(disk.data(), sizeof(float), disk.size(), fp) == disk.size() &&
              fwrite(n.data(), sizeof(short), n.size(), fp) == n.size();
    return fclose(fp) == 0 && ok;
}

/* one colour phase: the launch of start.cu:241-245, a single block of (cps/2)^3 threads */
static void run_phase(std::vector<float>& disk, std::vector<short>& n, int offset[3], uint32_t sweep,
                      uint64_t seed) {
    blockDim = {kCps / 2, kCps / 2, kCps / 2};
    gridDim = {1, 1, 1};
    blockIdx = {0, 0, 0};
    ref_barrier_on = false;
    for (int tz = 0; tz < kCps / 2; ++tz)
        for (int ty = 0; ty < kCps / 2; ++ty)
            for (int tx = 0; tx < kCps / 2; ++tx) {
                threadIdx = {tx, ty, tz};
                const int cell = (2 * tx + offset[0]) + kCps * ((2 * ty + offset[1]) + kCps * (2 * tz + offset[2]));
                const int count = n[cell];
                ref_rng_begin((uint32_t)cell, count, sweep, seed);
                subsweep_kernel(disk.data(), n.data(), offset);
                ref_rng_end(count, kMoves);
            }
}

/* Whether every cell's count after the shift stays within nmax: a cell keeps its particles whose
 * coordinate along f, taken from the cell's lower face and reduced by d, lies in (0, w], and takes
 * from its neighbour on the side of d's sign those that the neighbour does not keep. */
static bool new_counts_fit(const std::vector<float>& disk, const std::vector<short>& n, int f, float d) {
    const float half = ((float)kCps * kW) / 2.0f;
    std::vector<int> kept(kCells, 0);
    for (int c = 0; c < kCells; ++c) {
        const int cid[3] = {c % kCps, (c / kCps) % kCps, c / (kCps * kCps)};
        const float lower = cid[f] * kW - half;
        for (int i = 0; i < n[c]; ++i) {
            const float t = (disk[(size_t)c * 3 * kNmax + f * kNmax + i] - lower) - d;
            if (t > 0 && t <= kW) ++kept[c];
        }
    }
    const int stride[3] = {1, kCps, kCps * kCps};
    for (int c = 0; c < kCells; ++c) {
        const int along = (c / stride[f]) % kCps;
        const int nb_along = (along + (d <= 0 ? kCps - 1 : 1)) % kCps;
        const int nb = c + (nb_along - along) * stride[f];
        if (kept[c] + (n[nb] - kept[nb]) > kNmax) return false;
    }
    return true;
}

/* one shiftCells: the launch of start.cu:255, a single block of cps^3 threads */
static void run_shift(std::vector<float>& disk, std::vector<short>& n, int f, float d) {
    blockDim = {kCps, kCps, kCps};
    gridDim = {1, 1, 1};
    pthread_barrier_init(&ref_barrier, nullptr, (unsigned)kCells);
    ref_barrier_on = true;
    std::vector<std::thread> threads;
    threads.reserve(kCells);
    for (int c = 0; c < kCells; ++c)
        threads.emplace_back([&, c] {
            threadIdx = {c % kCps, (c / kCps) % kCps, c / (kCps * kCps)};
            blockIdx = {0, 0, 0};
            shiftCells(disk.data(), n.data(), f, d);
        });
    for (auto& t : threads) t.join();
    ref_barrier_on = false;
    pthread_barrier_destroy(&ref_barrier);
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "info")) {
        printf("cps %d nmax %d n_moves %d w %08x sigma %08x beta %08x\n", kCps, kNmax, kMoves, pmc_fbits(kW),
               pmc_fbits(REF_SIGMA), pmc_fbits(REF_BETA));
        return 0;
    }
    std::vector<float> disk;
    std::vector<short> n;
    if (argc == 9 && !strcmp(argv[1], "phase")) {
        int offset[3] = {atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
        for (int k = 0; k < 3; ++k)
            if (offset[k] != 0 && offset[k] != 1) return fail("offset components are 0 or 1");
        if (!read_state(argv[2], disk, n)) return fail("cannot read the input state (size, or a count outside 0..nmax)");
        run_phase(disk, n, offset, (uint32_t)strtoul(argv[7], nullptr, 0), strtoull(argv[8], nullptr, 0));
        return write_state(argv[3], disk, n) ? 0 : fail("cannot write the output state");
    }
    if (argc == 6 && !strcmp(argv[1], "shift")) {
        const int f = atoi(argv[4]);
        if (f < 0 || f > 2) return fail("f is 0, 1 or 2");
        const float d = pmc_bitsf((uint32_t)strtoul(argv[5], nullptr, 16));
        if (!read_state(argv[2], disk, n)) return fail("cannot read the input state (size, or a count outside 0..nmax)");
        if (!new_counts_fit(disk, n, f, d)) {
            fprintf(stderr, "ref_harness: a cell would exceed nmax: the reference overruns its local array there\n");
            return 3;
        }
        run_shift(disk, n, f, d);
        return write_state(argv[3], disk, n) ? 0 : fail("cannot write the output state");
    }
    fprintf(stderr, "usage: %s info | phase IN OUT ox oy oz sweep seed | shift IN OUT f dbits\n", argv[0]);
    return 2;
}

/* ---- the reference's program text, from the reference tree -------------------------------------
 * Its configuration macros have one-letter and common names (w, L, beta, sigma, nmax), so they are
 * defined only here, after everything of ours.  beta is a double in the reference (start.cu:16) and
 * the product beta * dE is formed in double; its value is the library's float beta widened. */
#define L ((float)(REF_CPS) * (REF_W))
#define beta ((double)(REF_BETA))
#define cellsPerSide (REF_CPS)
#define CPS2 ((REF_CPS) * (REF_CPS))
#define CPS3 ((REF_CPS) * (REF_CPS) * (REF_CPS))
#define w (REF_W)
#define nmax (REF_NMAX)
#define n_M (REF_NM)
#define sigma (REF_SIGMA)

#pragma GCC diagnostic ignored "-Wunused-variable"
#pragma GCC diagnostic ignored "-Wunused-parameter"
#pragma GCC diagnostic ignored "-Wmaybe-uninitialized"
#pragma GCC diagnostic ignored "-Wuninitialized"
#include "subsweep.h"
#include "shiftCells.h"
