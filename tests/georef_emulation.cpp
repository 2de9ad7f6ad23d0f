// ssrs_amd/csrc/georef.hip on the CPU (tests/test_warp_emulation.py): the kernel's logic -- cell ownership, the scalar
// tail and the packed stores, the gather's indices -- through tests/hip_host_stub, one OS thread per GPU thread.  What the
// stub lacks is supplied here.  A ballot sees one lane only, so the uncovered COUNT is not what the device gives and is
// not checked; the gpu-marked tests cover it.  Buffers are allocated at their exact sizes, so a build with
// -fsanitize=address sees any access outside them.
//   argv: src.bin src_type src_rows src_cols lon0 lat0 dlon dlat nodata|nan west south res dst_type rows cols out_prefix
//         offset_elements, then the eight inputs of SsrsProjection
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

inline double __longlong_as_double(long long v)
{
    double d;
    std::memcpy(&d, &v, sizeof d);
    return d;
}
inline unsigned long long __ballot(bool b) { return b ? 1ull : 0ull; }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v)
{
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
}

#include "../ssrs_amd/csrc/georef.hip"

namespace ssrs {
static char message[512];
char *error_buffer() { return message; }
int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(message, sizeof message, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace ssrs

static bool dump(const char *prefix, const char *what, const void *data, size_t size, size_t n)
{
    char name[1024];
    std::snprintf(name, sizeof name, "%s_%s.bin", prefix, what);
    FILE *f = std::fopen(name, "wb");
    const bool ok = f && std::fwrite(data, size, n, f) == n;
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 26) return 2;
    const int src_type = std::atoi(argv[2]), sr = std::atoi(argv[3]), sc = std::atoi(argv[4]);
    const double lon0 = std::atof(argv[5]), lat0 = std::atof(argv[6]), dlon = std::atof(argv[7]), dlat = std::atof(argv[8]);
    const double nodata = std::strcmp(argv[9], "nan") ? std::atof(argv[9]) : __builtin_nan("");
    const double west = std::atof(argv[10]), south = std::atof(argv[11]), res = std::atof(argv[12]);
    const int dst_type = std::atoi(argv[13]), rows = std::atoi(argv[14]), cols = std::atoi(argv[15]);
    const size_t off = static_cast<size_t>(std::atoi(argv[17]));
    SsrsProjection p{};
    double *in[8] = {&p.a, &p.e2, &p.lat_1, &p.lat_2, &p.lat_0, &p.lon_0, &p.x_0, &p.y_0};
    for (int k = 0; k < 8; ++k) *in[k] = std::atof(argv[18 + k]);
    if (ssrs_projection_init_albers(&p)) return 4;
    const size_t ssz = src_type ? 8 : 4, dsz = dst_type ? 8 : 4, n = static_cast<size_t>(rows) * cols;
    void *src = std::malloc(ssz * sr * sc);
    FILE *f = std::fopen(argv[1], "rb");
    if (!src || !f || std::fread(src, ssz, static_cast<size_t>(sr) * sc, f) != static_cast<size_t>(sr) * sc) return 3;
    std::fclose(f);
    // `off` elements in front: off = 1 leaves the bases unaligned, which takes the one-by-one stores
    char *dst = static_cast<char *>(std::malloc(dsz * (n + off)));
    double *lon = static_cast<double *>(std::malloc(8 * (n + off))), *lat = static_cast<double *>(std::malloc(8 * (n + off)));
    unsigned long long uncovered = 0;
    const int rc = ssrs_warp_lonlat_raster(src, src_type, sr, sc, lon0, lat0, dlon, dlat, nodata, &p, west, south, res,
                                           dst + dsz * off, dst_type, lon + off, lat + off, &uncovered, rows, cols, nullptr);
    if (rc) {
        std::fprintf(stderr, "%s\n", ssrs::message);
        return 5;
    }
    const bool ok = dump(argv[16], "dst", dst + dsz * off, dsz, n) && dump(argv[16], "lon", lon + off, 8, n) &&
                    dump(argv[16], "lat", lat + off, 8, n);
    std::free(src);
    std::free(dst);
    std::free(lon);
    std::free(lat);
    return ok ? 0 : 6;
}
