// The WGS-84 transverse Mercator projection (UTM) in fp64, both ways, shared by the DSM extraction
// (dsm.hip: forward), the ground-grid rays (ortho.hip: inverse) and the orthorectification
// (rectify.hip: both).  Krüger's series to 6th order in n; oracle/dsm_ref.py states the forward series
// in numpy and tests/ortho_numpy.py the inverse one.
#pragma once
#include <cmath>

#include "common.h"

namespace spn {

// WGS-84 transverse Mercator (UTM) by Krüger's series to 6th order in n (utm_krueger in
// oracle/dsm_ref.py is the same arithmetic in numpy)
__device__ __forceinline__ void utm_forward(double lat_deg, double lon_deg, int zone, int south, double* e, double* nn) {
    const double a = 6378137.0, f = 1.0 / 298.257223563, k0 = 0.9996;
    const double n = f / (2.0 - f), n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
    const double A = a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0);
    const double al[6] = {n / 2.0 - 2.0 * n2 / 3.0 + 5.0 * n3 / 16.0 + 41.0 * n4 / 180.0 - 127.0 * n5 / 288.0 +
                              7891.0 * n6 / 37800.0,
                          13.0 * n2 / 48.0 - 3.0 * n3 / 5.0 + 557.0 * n4 / 1440.0 + 281.0 * n5 / 630.0 -
                              1983433.0 * n6 / 1935360.0,
                          61.0 * n3 / 240.0 - 103.0 * n4 / 140.0 + 15061.0 * n5 / 26880.0 + 167603.0 * n6 / 181440.0,
                          49561.0 * n4 / 161280.0 - 179.0 * n5 / 168.0 + 6601661.0 * n6 / 7257600.0,
                          34729.0 * n5 / 80640.0 - 3418889.0 * n6 / 1995840.0,
                          212378941.0 * n6 / 319334400.0};
    const double deg = M_PI / 180.0;
    const double phi = lat_deg * deg;
    const double lam = (lon_deg - (6.0 * zone - 183.0)) * deg;
    const double c = 2.0 * sqrt(n) / (1.0 + n);
    const double t = sinh(atanh(sin(phi)) - c * atanh(c * sin(phi)));
    const double xi = atan2(t, cos(lam));
    const double eta = atanh(sin(lam) / sqrt(1.0 + t * t));
    double se = eta, sn = xi;
    for (int j = 1; j <= 6; ++j) {
        se += al[j - 1] * cos(2.0 * j * xi) * sinh(2.0 * j * eta);
        sn += al[j - 1] * sin(2.0 * j * xi) * cosh(2.0 * j * eta);
    }
    *e = 500000.0 + k0 * A * se;
    *nn = (south ? 10000000.0 : 0.0) + k0 * A * sn;
}

// WGS-84 UTM (E, N) → geodetic (lat, lon) in degrees
__device__ __forceinline__ void utm_inverse(double e, double nn, int zone, int south, double* lat_deg, double* lon_deg) {
    const double a = 6378137.0, f = 1.0 / 298.257223563, k0 = 0.9996;
    const double n = f / (2.0 - f), n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
    const double A = a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0);
    const double be[6] = {n / 2.0 - 2.0 * n2 / 3.0 + 37.0 * n3 / 96.0 - n4 / 360.0 - 81.0 * n5 / 512.0 +
                              96199.0 * n6 / 604800.0,
                          n2 / 48.0 + n3 / 15.0 - 437.0 * n4 / 1440.0 + 46.0 * n5 / 105.0 - 1118711.0 * n6 / 3870720.0,
                          17.0 * n3 / 480.0 - 37.0 * n4 / 840.0 - 209.0 * n5 / 4480.0 + 5569.0 * n6 / 90720.0,
                          4397.0 * n4 / 161280.0 - 11.0 * n5 / 504.0 - 830251.0 * n6 / 7257600.0,
                          4583.0 * n5 / 161280.0 - 108847.0 * n6 / 3991680.0,
                          20648693.0 * n6 / 638668800.0};
    const double xi = (nn - (south ? 10000000.0 : 0.0)) / (k0 * A);
    const double eta = (e - 500000.0) / (k0 * A);
    double xp = xi, ep = eta;
    for (int j = 1; j <= 6; ++j) {
        xp -= be[j - 1] * sin(2.0 * j * xi) * cosh(2.0 * j * eta);
        ep -= be[j - 1] * cos(2.0 * j * xi) * sinh(2.0 * j * eta);
    }
    const double sh = sinh(ep), cxp = cos(xp);
    const double taup = sin(xp) / sqrt(sh * sh + cxp * cxp);   // tan of the conformal latitude
    const double lam = atan2(sh, cxp);
    // τ from τ' = τ·sqrt(1 + σ²) − σ·sqrt(1 + τ²), σ = sinh(e·atanh(e·τ / sqrt(1 + τ²))): Newton from
    // τ = τ' converges quadratically (two or three steps); stop when a step no longer moves τ
    const double e2 = f * (2.0 - f), ecc = sqrt(e2);
    double tau = taup;
    for (int it = 0; it < 8; ++it) {
        const double t1 = sqrt(1.0 + tau * tau);
        const double sg = sinh(ecc * atanh(ecc * tau / t1));
        const double tp = tau * sqrt(1.0 + sg * sg) - sg * t1;
        const double dt = (taup - tp) / sqrt(1.0 + tp * tp) * (1.0 + (1.0 - e2) * tau * tau) / ((1.0 - e2) * t1);
        tau += dt;
        if (!(fabs(dt) > 1e-16 * fmax(1.0, fabs(tau)))) break;
    }
    *lat_deg = atan(tau) * (180.0 / M_PI);
    *lon_deg = lam * (180.0 / M_PI) + (6.0 * zone - 183.0);
}

}  // namespace spn
