// Device RPC localisation and WGS-84 ECEF shared by the ray generator (rays.hip) and the training-set
// kernels (dataset.hip): one pixel → one un-normalised ray, datasets/satellite_scene.py:21-68.
//
// Localization (image → ground) restates rpcm's iterative inversion of the RPC00B projection
// in fp64 (see oracle/rpc_ref.py): project the estimate and two offset points (lon + EPS,
// lat + EPS), decompose the image residual on the offset vectors, step; EPS = 2 then 0.1; stop
// at a squared normalised residual < 1e-18 (rpcm iterates its whole batch until every point
// converges; here each pixel stops on its own and takes two extra refinement steps).
#pragma once
#include "common.h"

namespace spn {

struct RpcCam {
    double off[10];  // row_offset col_offset lat_offset lon_offset alt_offset row_scale col_scale lat_scale lon_scale alt_scale
    double rn[20], rd[20], cn[20], cd[20];
    double min_alt, max_alt;
};

// the 90 packed doubles of the C ABI → RpcCam, rescaled as utils.rescale_rpc(rpc, 1/downscale)
inline void rpc_unpack(RpcCam& a, const double* rpc, double downscale, double min_alt, double max_alt) {
    for (int k = 0; k < 10; ++k) a.off[k] = rpc[k];
    for (int k = 0; k < 20; ++k) {
        a.rn[k] = rpc[10 + k];
        a.rd[k] = rpc[30 + k];
        a.cn[k] = rpc[50 + k];
        a.cd[k] = rpc[70 + k];
    }
    const double s = 1.0 / downscale;
    a.off[5] *= s;
    a.off[6] *= s;
    a.off[0] *= s;
    a.off[1] *= s;
    a.min_alt = min_alt;
    a.max_alt = max_alt;
}

__device__ __forceinline__ double rpoly(const double* c, double x, double y, double z) {
    // x = lat, y = lon, z = alt (normalised); RPC00B monomial order
    return c[0] + c[1] * y + c[2] * x + c[3] * z + c[4] * y * x + c[5] * y * z + c[6] * x * z + c[7] * y * y +
           c[8] * x * x + c[9] * z * z + c[10] * x * y * z + c[11] * y * y * y + c[12] * y * x * x +
           c[13] * y * z * z + c[14] * y * y * x + c[15] * x * x * x + c[16] * x * z * z + c[17] * y * y * z +
           c[18] * x * x * z + c[19] * z * z * z;
}

__device__ __forceinline__ void proj_n(const RpcCam& a, double lat, double lon, double alt, double& col, double& row) {
    col = rpoly(a.cn, lat, lon, alt) / rpoly(a.cd, lat, lon, alt);
    row = rpoly(a.rn, lat, lon, alt) / rpoly(a.rd, lat, lon, alt);
}

// The iteration itself, over any projection proj(lat, lon, an, col, row) on normalised coordinates: normalised
// image (cn, rn) at normalised altitude an → normalised (lon, lat).  Stated once: localize below runs it on an
// RpcCam, localize_packed (csrc/rectify_cell.h) on a packed camera table.
template <class Proj>
__device__ __forceinline__ void localize_n(Proj proj, double cn, double rn, double an, double& lon_n, double& lat_n) {
    double lon = -1.0, lat = -1.0, eps = 2.0;
    int extra = -1;
    for (int it = 0; it <= 100; ++it) {
        double x0, y0;
        proj(lat, lon, an, x0, y0);
        const double res = (x0 - cn) * (x0 - cn) + (y0 - rn) * (y0 - rn);
        if (res < 1e-18) {
            if (extra < 0) extra = 2;
            if (extra-- == 0) break;
        }
        double x1, y1, x2, y2;
        proj(lat, lon + eps, an, x1, y1);
        proj(lat + eps, lon, an, x2, y2);
        const double e1x = x1 - x0, e1y = y1 - y0, e2x = x2 - x0, e2y = y2 - y0;
        const double ux = cn - x0, uy = rn - y0;
        const double a1 = (ux * e1x + uy * e1y) / (e1x * e1x + e1y * e1y);
        const double a2 = (ux * e2x + uy * e2y) / (e2x * e2x + e2y * e2y);
        lon += a1 * eps;
        lat += a2 * eps;
        eps = 0.1;
    }
    lon_n = lon;
    lat_n = lat;
}

// normalised image (cn, rn) at normalised altitude an → degrees (lon, lat)
__device__ inline void localize(const RpcCam& a, double cn, double rn, double an, double& lon_d, double& lat_d) {
    double lon, lat;
    localize_n([&a](double la, double lo, double al, double& x, double& y) { proj_n(a, la, lo, al, x, y); }, cn, rn, an, lon, lat);
    lon_d = lon * a.off[8] + a.off[3];
    lat_d = lat * a.off[7] + a.off[2];
}

__device__ inline void ecef(double lat_deg, double lon_deg, double alt, double& x, double& y, double& z) {
    const double A = 6378137.0, Bm = 6356752.314245;
    const double ba = (Bm * Bm) / (A * A);
    const double e2 = 1.0 - ba;
    const double la = lat_deg * (M_PI / 180.0), lo = lon_deg * (M_PI / 180.0);
    const double sl = sin(la);
    const double N = A / sqrt(1.0 - e2 * (sl * sl));
    x = (N + alt) * cos(la) * cos(lo);
    y = (N + alt) * cos(la) * sin(lo);
    z = (ba * N + alt) * sl;
}

// the ray of pixel (col, row): v = [o (ECEF rounded to fp32), d, near = 0, far = ‖far − near‖]
__device__ inline void rpc_ray(const RpcCam& a, double col, double row, float (&v)[8]) {
    const double cnm = (col - a.off[1]) / a.off[6], rnm = (row - a.off[0]) / a.off[5];
    double lon, lat, xn, yn, zn, xf, yf, zf;
    localize(a, cnm, rnm, (a.max_alt - a.off[4]) / a.off[9], lon, lat);
    ecef(lat, lon, a.max_alt, xn, yn, zn);
    localize(a, cnm, rnm, (a.min_alt - a.off[4]) / a.off[9], lon, lat);
    ecef(lat, lon, a.min_alt, xf, yf, zf);
    const double dx = xf - xn, dy = yf - yn, dz = zf - zn;
    const double nrm = sqrt((dx * dx + dy * dy) + dz * dz);
    v[0] = (float)xn;
    v[1] = (float)yn;
    v[2] = (float)zn;
    v[3] = (float)(dx / nrm);
    v[4] = (float)(dy / nrm);
    v[5] = (float)(dz / nrm);
    v[6] = 0.f;
    v[7] = (float)nrm;
}

// satellite_scene.py:415-425 on one ray, in fp32: the 0.5 m fp32 quantisation of ECEF at 5.45e6 m is
// reproduced, not removed
__device__ __forceinline__ void normalize_ray(float (&v)[8], const float (&center)[3], float range) {
    for (int k = 0; k < 3; ++k) v[k] = __fdiv_rn(__fsub_rn(v[k], center[k]), range);
    v[6] = __fdiv_rn(v[6], range);
    v[7] = __fdiv_rn(v[7], range);
}

}  // namespace spn
