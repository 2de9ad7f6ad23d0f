// Host-only print-out of the blur's radius and weights (ssrs_amd/csrc/gauss.h), for tests/test_thermals_ref_host.py to
// compare with smooth_ref.weights bit for bit.  One line per sigma given on the command line:
//   <sigma as given> <radius> <2 radius + 1 weights, each as the 16 hex digits of its f64 bits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ssrs_amd/csrc/gauss.h"

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        const double sigma = std::strtod(argv[a], nullptr);
        const int radius = blur_radius(sigma);
        const std::vector<double> w = blur_weights(sigma, radius);
        std::printf("%s %d", argv[a], radius);
        for (double v : w) {
            uint64_t bits;
            std::memcpy(&bits, &v, 8);
            std::printf(" %016llx", static_cast<unsigned long long>(bits));
        }
        std::printf("\n");
    }
    return 0;
}
