// Ground-grid rays and their reduction (include/spnerf_amd_ortho.h): the DSM and the true-ortho
// products of S-NeRF / EO-NeRF, one vertical ray per cell of a UTM grid instead of one camera's
// point cloud pushed through the forward projection and a rasteriser (csrc/dsm.hip).
//  * k_ortho_rays — one thread per sub-ray: (E, N) → (lat, lon) by utm_inverse
//    (csrc/utm.h) — Krüger's series to 6th order in n with the β coefficients of Karney, "Transverse
//    Mercator with an accuracy of a few nanometers" (2011), eq. (36), then Newton steps on
//    τ = tan φ from the conformal to the geodetic latitude (eqs. (19)-(21)) — then the two ECEF
//    points at max_alt / min_alt (csrc/rpc.h: the reference's geodetic_to_ecef) and the normalised
//    ray.  fp64 up to the store: the camera rays round ECEF to fp32 before centring
//    (csrc/rays.hip), half a metre at 6.4e6 m — a whole cell here, so it is not reproduced.
//  * k_ortho_reduce — one thread per output value: the s² contiguous sub-rays of a cell summed in
//    fp64 in index order, one division, one cast.
//  * k_ortho_classes — one thread per cell: torch.argmax's rule over the reduced mean logits.
// HBM-trivial next to the render between them (32 or 44 B per ray out; ≤ 4 B per value in).
#include <cmath>

#include "../../include/spnerf_amd_ortho.h"
#include "rpc.h"
#include "utm.h"

namespace spn {

struct OrthoRayArgs {
    double xoff, ytop, res;
    int xsize, s, row0, zone, south;
    int64_t n;
    double min_alt, max_alt, cx, cy, cz, range;
    float sun[3];
    float* out;
    int stride;
};

__global__ __launch_bounds__(256) void k_ortho_rays(OrthoRayArgs g) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= g.n) return;
    // r = ((jj·xsize + i)·s + a)·s + b, jj the row within the band
    const int b = (int)(r % g.s), a = (int)((r / g.s) % g.s);
    const int64_t cell = r / ((int64_t)g.s * g.s);
    const int i = (int)(cell % g.xsize);
    const int64_t j = g.row0 + cell / g.xsize;
    const double E = g.xoff + ((double)i + ((double)b + 0.5) / (double)g.s) * g.res;
    const double N = g.ytop - ((double)j + ((double)a + 0.5) / (double)g.s) * g.res;
    double lat, lon, xn, yn, zn, xf, yf, zf;
    utm_inverse(E, N, g.zone, g.south, &lat, &lon);
    ecef(lat, lon, g.max_alt, xn, yn, zn);
    ecef(lat, lon, g.min_alt, xf, yf, zf);
    const double dx = xf - xn, dy = yf - yn, dz = zf - zn;
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    float* o = g.out + r * g.stride;
    o[0] = (float)((xn - g.cx) / g.range);
    o[1] = (float)((yn - g.cy) / g.range);
    o[2] = (float)((zn - g.cz) / g.range);
    o[3] = (float)(dx / len);
    o[4] = (float)(dy / len);
    o[5] = (float)(dz / len);
    o[6] = 0.0f;
    o[7] = (float)(len / g.range);
    if (g.stride == 11)
        for (int k = 0; k < 3; ++k) o[8 + k] = g.sun[k];
}

// out[v] for v = (m·cells + c)·width + w: the images are contiguous, so m·cells + c is one index
template <typename T>
__global__ __launch_bounds__(256) void k_ortho_reduce(const T* __restrict__ in, T* __restrict__ out, int64_t n_out, int width,
                                                      int s2) {
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v >= n_out) return;
    const int64_t cell = v / width;
    const int w = (int)(v % width);
    const T* p = in + cell * s2 * width + w;
    double acc = (double)p[0];
    for (int k = 1; k < s2; ++k) acc += (double)p[(int64_t)k * width];
    out[v] = (T)(acc / (double)s2);
}

__global__ __launch_bounds__(256) void k_ortho_classes(const float* __restrict__ logits, int64_t cells, int C,
                                                       int32_t* __restrict__ labels) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const float* p = logits + i * C;
    float best = p[0];
    int cls = 0;
    for (int c = 1; c < C; ++c) {
        const float m = p[c];
        if (best == best && (m > best || m != m)) {   // the first maximum; the first NaN stands
            best = m;
            cls = c;
        }
    }
    labels[i] = cls;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_ortho_abi_version(void) { return SPNERF_ORTHO_ABI_VERSION; }

extern "C" int32_t spnerf_ortho_rays(const spnerf_ortho_grid* grid, int32_t row0, int32_t n_rows, double min_alt,
                                     double max_alt, const double* center, double range, const float* sun, float* rays,
                                     int32_t ray_stride, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grid && center && rays, "ortho_rays: NULL grid, center or rays");
    SPN_ARG(grid->zone >= 1 && grid->zone <= 60, "ortho_rays: UTM zone %d", grid->zone);
    SPN_ARG(grid->supersample >= 1 && grid->supersample <= SPNERF_ORTHO_MAX_SUPERSAMPLE, "ortho_rays: supersample %d outside [1, %d]",
            grid->supersample, SPNERF_ORTHO_MAX_SUPERSAMPLE);
    SPN_ARG(grid->xsize > 0 && grid->ysize > 0, "ortho_rays: grid of %d x %d cells", grid->xsize, grid->ysize);
    SPN_ARG(grid->resolution > 0.0 && std::isfinite(grid->resolution), "ortho_rays: resolution %g", grid->resolution);
    SPN_ARG(std::isfinite(grid->xoff) && std::isfinite(grid->ytop), "ortho_rays: non-finite grid origin");
    SPN_ARG(max_alt > min_alt, "ortho_rays: max_alt %g must be above min_alt %g", max_alt, min_alt);
    SPN_ARG(range > 0.0, "ortho_rays: range %g", range);
    SPN_ARG(row0 >= 0 && n_rows >= 0 && (int64_t)row0 + n_rows <= grid->ysize, "ortho_rays: rows [%d, %lld) outside the grid's %d",
            row0, (long long)row0 + n_rows, grid->ysize);
    SPN_ARG(ray_stride == 8 || ray_stride == 11, "ortho_rays: ray_stride %d is neither 8 nor 11", ray_stride);
    SPN_ARG(ray_stride == 8 || sun, "ortho_rays: an 11-wide ray needs the sun direction");
    const int s = grid->supersample;
    OrthoRayArgs g{};
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution;
    g.xsize = grid->xsize; g.s = s; g.row0 = row0; g.zone = grid->zone; g.south = grid->south ? 1 : 0;
    SPN_ARG((int64_t)n_rows * grid->xsize <= 0x7fffffffLL * 256 / (s * s), "ortho_rays: %lld cells x %d sub-rays in one launch",
            (long long)n_rows * grid->xsize, s * s);
    g.n = (int64_t)n_rows * grid->xsize * s * s;
    g.min_alt = min_alt; g.max_alt = max_alt;
    g.cx = center[0]; g.cy = center[1]; g.cz = center[2]; g.range = range;
    if (ray_stride == 11)
        for (int k = 0; k < 3; ++k) g.sun[k] = sun[k];
    g.out = rays; g.stride = ray_stride;
    if (g.n == 0) return SPNERF_OK;
    ProfScope prof("ortho", st, 0.0, 4.0 * ray_stride * (double)g.n);
    hipLaunchKernelGGL(k_ortho_rays, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, g);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_ortho_reduce(const void* in, void* out, int64_t n_images, int64_t cells, int32_t width,
                                       int32_t supersample, int32_t dtype, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(in && out, "ortho_reduce: NULL planes");
    SPN_ARG(supersample >= 1 && supersample <= SPNERF_ORTHO_MAX_SUPERSAMPLE, "ortho_reduce: supersample %d outside [1, %d]",
            supersample, SPNERF_ORTHO_MAX_SUPERSAMPLE);
    SPN_ARG(n_images >= 0 && cells >= 0 && width > 0, "ortho_reduce: bad sizes (%lld images of %lld cells, width %d)",
            (long long)n_images, (long long)cells, width);
    SPN_ARG(dtype == 0 || dtype == 1, "ortho_reduce: dtype %d is neither 0 (fp32) nor 1 (fp64)", dtype);
    SPN_ARG(in != out, "ortho_reduce: the reduced planes cannot be the input planes");
    const int s2 = supersample * supersample;
    SPN_ARG(n_images == 0 || cells <= ((int64_t)1 << 38) / n_images / width,
            "ortho_reduce: %lld x %lld cells of width %d in one launch", (long long)n_images, (long long)cells, width);
    const int64_t n_out = n_images * cells * width;
    if (supersample == 1 || n_out == 0) return SPNERF_OK;
    const double bytes = (double)n_out * (s2 + 1) * (dtype ? 8.0 : 4.0);
    ProfScope prof("ortho", st, 0.0, bytes);
    const dim3 grid((unsigned)((n_out + 255) / 256));
    if (dtype)
        hipLaunchKernelGGL(k_ortho_reduce<double>, grid, dim3(256), 0, st, (const double*)in, (double*)out, n_out, width, s2);
    else
        hipLaunchKernelGGL(k_ortho_reduce<float>, grid, dim3(256), 0, st, (const float*)in, (float*)out, n_out, width, s2);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_ortho_classes(const float* logits, int64_t cells, int32_t n_classes, int32_t* labels,
                                        void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(logits && labels, "ortho_classes: NULL logits or labels");
    SPN_ARG(cells >= 0 && cells <= (int64_t)0x7fffffffLL * 256, "ortho_classes: cells %lld", (long long)cells);
    SPN_ARG(n_classes > 0, "ortho_classes: n_classes %d", n_classes);
    if (cells == 0) return SPNERF_OK;
    ProfScope prof("ortho", st, 0.0, (double)cells * (4.0 * n_classes + 4.0));
    hipLaunchKernelGGL(k_ortho_classes, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, logits, cells, n_classes, labels);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
