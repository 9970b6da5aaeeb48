// Stand-alone host program over the K2R_HD helpers of dcdf_amd/csrc/k2r_space.h (TEST INFRASTRUCTURE ONLY): the arithmetic the
// exact sum of dcdf_raster_reduce_space_batch rests on, run on a CPU -- built with -fsanitize=address,undefined by
// tests/test_reduce_space_host.py.  Reads commands from the file named on the command line, prints one line per command:
//   C k  (enc fbits n) * k   cells, each a record of its own (space_m, space_add_m, space_scale), folded in 192 bits and rounded:
//                            prints the sum's bits, then the bits of every cell's decoded value (from_fixed / (double)n)
//   E enc fbits n cnt        an elided piece: n's value x cnt selected cells (space_mul_m): prints the sum's bits
//   R k  (hi lo scale) * k   records as they are: prints the sum's bits
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dcdf_amd/csrc/k2r_space.h"

using namespace k2r;

static uint64_t bits_of(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}
static double widen(int32_t enc, uint32_t fbits, int64_t n) {  // reduce_widen (k2r_reduce.h) of n != 0
    switch (enc) {
        case ENC_I32: return (double)(int32_t)n;
        case ENC_I64: return (double)n;
        case ENC_F32: return (double)from_fixed_f32(n, fbits);
        default: return from_fixed_f64(n, fbits);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char cmd;
    while (std::fscanf(f, " %c", &cmd) == 1) {
        U192 acc{0, 0, 0};
        if (cmd == 'C') {
            size_t k;
            if (std::fscanf(f, "%zu", &k) != 1) return 3;
            std::vector<uint64_t> xs;
            for (size_t i = 0; i < k; i++) {
                int32_t enc;
                uint32_t fbits;
                int64_t n;
                if (std::fscanf(f, "%" SCNd32 " %" SCNu32 " %" SCNd64, &enc, &fbits, &n) != 3) return 3;
                SpacePartial p{0, 0, 0.0, 0.0, 1, space_scale(enc, fbits)};
                space_add_m(p.hi, p.lo, space_m(enc, n));
                u192_add(acc, space_scaled(p.hi, p.lo, p.scale));
                xs.push_back(bits_of(widen(enc, fbits, n)));
            }
            std::printf("%016" PRIx64, bits_of(space_round(acc)));
            for (uint64_t x : xs) std::printf(" %016" PRIx64, x);
            std::printf("\n");
        } else if (cmd == 'E') {
            int32_t enc;
            uint32_t fbits, cnt;
            int64_t n;
            if (std::fscanf(f, "%" SCNd32 " %" SCNu32 " %" SCNd64 " %" SCNu32, &enc, &fbits, &n, &cnt) != 4) return 3;
            uint64_t hi = 0, lo = 0;
            space_mul_m(hi, lo, space_m(enc, n), cnt);
            u192_add(acc, space_scaled(hi, lo, space_scale(enc, fbits)));
            std::printf("%016" PRIx64 "\n", bits_of(space_round(acc)));
        } else if (cmd == 'R') {
            size_t k;
            if (std::fscanf(f, "%zu", &k) != 1) return 3;
            for (size_t i = 0; i < k; i++) {
                uint64_t hi, lo;
                uint32_t scale;
                if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu32, &hi, &lo, &scale) != 3) return 3;
                u192_add(acc, space_scaled(hi, lo, scale));
            }
            std::printf("%016" PRIx64 "\n", bits_of(space_round(acc)));
        } else {
            return 3;
        }
    }
    std::fclose(f);
    return 0;
}
