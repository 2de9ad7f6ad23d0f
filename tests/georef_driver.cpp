// ssrs_amd/csrc/georef.h in a plain C++ program (tests/test_georef_host.py): reads from stdin
//   a e2 lat_1 lat_2 lat_0 lon_0 x_0 y_0
//   npts, then npts lines "lon lat", then npts lines "x y"
// and prints "n C rho0 e", the forward projection of every (lon, lat) and the inverse of every (x, y), all %.17g.
// "invalid" instead when the parameters give no cone.  Exit status 2 for input it cannot read.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../ssrs_amd/csrc/georef.h"

int main()
{
    SsrsProjection p{};
    if (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf", &p.a, &p.e2, &p.lat_1, &p.lat_2, &p.lat_0, &p.lon_0, &p.x_0, &p.y_0) != 8)
        return 2;
    if (!ssrs::albers_init(&p)) {
        std::printf("invalid\n");
        return 0;
    }
    std::printf("%.17g %.17g %.17g %.17g\n", p.n, p.C, p.rho0, p.e);
    int npts = 0;
    if (std::scanf("%d", &npts) != 1 || npts < 0 || npts > (1 << 24)) return 2;
    std::vector<double> u(npts), v(npts);
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < npts; ++k)
            if (std::scanf("%lf %lf", &u[k], &v[k]) != 2) return 2;
        for (int k = 0; k < npts; ++k) {
            double s, t;
            if (pass == 0)
                ssrs::albers_forward(p, u[k], v[k], s, t);
            else
                ssrs::albers_inverse(p, u[k], v[k], s, t);
            std::printf("%.17g %.17g\n", s, t);
        }
    }
    return 0;
}
