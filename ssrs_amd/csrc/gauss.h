// The 1-D Gaussian of scipy.ndimage.gaussian_filter, on the host in f64: shared by the zero-padded blur of the
// thermal fields (thermals.hip) and the reflected blur of the orographic updraft (smooth.hip), so that both use
// the very same radius and weights.
#pragma once
#include <cmath>
#include <vector>

// scipy.ndimage._gaussian_kernel1d: radius = int(truncate * sigma + 0.5), truncate = 4
static int blur_radius(double sigma) { return static_cast<int>(4.0 * sigma + 0.5); }

static std::vector<double> blur_weights(double sigma, int radius)
{
    std::vector<double> w(2 * radius + 1);
    double sum = 0.0;
    for (int k = -radius; k <= radius; ++k) { w[k + radius] = std::exp(-0.5 / (sigma * sigma) * k * k); sum += w[k + radius]; }
    for (double &v : w) v /= sum;
    return w;
}
