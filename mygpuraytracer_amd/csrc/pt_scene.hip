// pt_scene.hip -- scene preparation as host-only code (pt_scene.h): what ptx_create derives from the caller's geoms and materials before
// it uploads, the camera's per-tile geom masks, and the ptx_debug_* entry points that are host arithmetic only.  No __global__ function
// and no hip* runtime call, so a CPU program links this object without a GPU; compiled as HIP with pt_engine.hip's flags because the
// tabulated normals and ptx_debug_bvh_check's walks are pt_device.h's own functions compiled for the host: exact at every level.
#include <string>

#include "pt_scene.h"
#include "pt_kernels.h"

extern "C" void ptx_internal_set_error(const char *msg);

static int set_error(int code, const std::string &msg) { ptx_internal_set_error(msg.c_str()); return code; }

namespace ptd {
void camera_to_device(const ptx_camera &c, DCamera &d) {
    d.resx = c.resolution[0]; d.resy = c.resolution[1];
    memcpy(d.position, c.position, 12); memcpy(d.lookAt, c.lookAt, 12); memcpy(d.view, c.view, 12);
    memcpy(d.up, c.up, 12); memcpy(d.right, c.right, 12); memcpy(d.fov, c.fov, 8); memcpy(d.pixelLength, c.pixelLength, 8);
}

// Conservative world-space box of a geom for the candidate pre-test of intersectSceneCull: the transformed unit cube
// (which also contains the radius-0.5 sphere) or the transformed mesh vertices, evaluated in double and inflated by
// 1e-3 + 1e-4 * |coordinate| -- three orders of magnitude more than the fp32 error of the exact tests or of the slab
// pre-test itself, so a ray the exact test would report as a hit always reaches the box.  Anything non-finite gives an
// unbounded box (never culled).
void make_world_aabb(const DGeom &d, const std::vector<float> &faces, float out6[6]) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    bool ok = true;
    auto add = [&](double x, double y, double z) {
        for (int r = 0; r < 3; r++) {
            double v = (double)d.xf[0 * 4 + r] * x + (double)d.xf[1 * 4 + r] * y + (double)d.xf[2 * 4 + r] * z + (double)d.xf[3 * 4 + r];
            if (!(v == v) || v > 1e30 || v < -1e30) ok = false;
            lo[r] = std::min(lo[r], v); hi[r] = std::max(hi[r], v);
        }
    };
    if (d.type == G_OBJ) {
        if (d.faceCount == 0) ok = false;
        for (int j = 0; j < d.faceCount; j++)
            for (int k = 0; k < 3; k++) {
                const float *p = &faces[((size_t)d.faceStart + j) * 15 + k * 5];
                add(p[0], p[1], p[2]);
            }
    } else {
        for (int c = 0; c < 8; c++) add((c & 1) ? 0.5 : -0.5, (c & 2) ? 0.5 : -0.5, (c & 4) ? 0.5 : -0.5);
    }
    for (int r = 0; r < 3; r++) {
        if (!ok) { out6[r] = -INFINITY; out6[3 + r] = INFINITY; continue; }
        double m = 1e-3 + 1e-4 * std::max(std::fabs(lo[r]), std::fabs(hi[r]));
        out6[r] = nextafterf((float)(lo[r] - m), -INFINITY);
        out6[3 + r] = nextafterf((float)(hi[r] + m), INFINITY);
    }
}

// Which material bins' records must carry the incoming direction to the next bounce -- scatterRay (pt_device.h) reads it in its
// reflective and refractive branches and for every hit on an OBJ geom (Schlick's cosine), never for a diffuse cube or sphere hit --
// and which bins' hits are all cube hits (the material is on cubes only): their records carry a code for the cube's tabulated normal
// instead of the normal.  The next bounce tells the kinds of record apart by sorted position, at most two ranges each, so a mask keeps
// at most two runs of set bits: gaps between the runs of the first are FILLED (a direction more is harmless), runs beyond the second
// of the other are CLEARED.  nmaterials <= 64 bins (bin = nmaterials - 1 - material when sorting, else one bin).
void record_masks(int nmaterials, const DMaterial *mats, int ngeoms, const int *geom_type, const int *geom_material, bool sort,
                  unsigned long long &dir_bins, unsigned long long &ntab_bins) {
    unsigned long long need = 0, cubes = 0;
    const int nbins = sort ? nmaterials : 1;
    for (int m = 0; m < nmaterials; m++) {
        bool nd = mats[m].hasReflective > 0 || mats[m].hasRefractive > 0, on_cube = false, on_other = false;
        for (int i = 0; i < ngeoms; i++)
            if (geom_material[i] == m) { nd = nd || geom_type[i] == G_OBJ; (geom_type[i] == G_CUBE ? on_cube : on_other) = true; }
        const int b = sort ? nmaterials - 1 - m : 0;
        if (nd) need |= 1ull << b;
        if (on_cube && !on_other && sort) cubes |= 1ull << b;
    }
    auto runs = [&](unsigned long long mask) { int n = 0; for (int b = 0; b < nbins; b++) n += ((mask >> b) & 1) && !(b && ((mask >> (b - 1)) & 1)); return n; };
    while (runs(need) > 2) {                          // fill the gap behind the first run
        int b = 0;
        while (!((need >> b) & 1)) b++;
        while ((need >> b) & 1) b++;
        need |= 1ull << b;
    }
    while (runs(cubes) > 2) cubes &= ~(1ull << (63 - __builtin_clzll(cubes)));      // drop the highest set bin
    dir_bins = need; ntab_bins = cubes;
}

// The same box as the device's candidate pre-test reads it (cullMask): centre and half extent.  The half extent grows by what the two
// roundings can lose (half an ulp of the centre, half an ulp of itself) and then some; an unbounded box is centre 0, half extent inf.
void world_box_centre_half(const float lohi8[8], float out8[8]) {
    for (int r = 0; r < 3; r++) {
        const double lo = lohi8[r], hi = lohi8[4 + r];
        if (!(lo > -1e30 && hi < 1e30)) { out8[r] = 0.f; out8[4 + r] = INFINITY; continue; }
        const float c = (float)(0.5 * (lo + hi));
        const double h = std::max(hi - (double)c, (double)c - lo);
        out8[r] = c;
        out8[4 + r] = nextafterf((float)(h + 2e-7 * (std::fabs((double)c) + h)), INFINITY);
    }
    out8[3] = out8[7] = 0.f;
}

// Which geoms can the camera rays of a tile reach at all?  Per geom the pixel rectangle that its conservative world box projects
// into (double precision, widened by the antialiasing jitter and two more pixels); a corner at or behind the eye plane makes it the
// whole frame.  A tile is 256 consecutive OWNED pixels: one span of a row, or -- when it wraps -- whole rows.  Bit g of a tile's
// word is cleared only when geom g's rectangle misses the tile's: a superset of what any of its rays can hit, so the candidate
// masks built from it (cullMask<SUBSET>) hold exactly the bits the full loop would set for those rays.  Recomputed when the camera
// changes; not where the candidate masks are off.
// With depth of field (generateRay: src/pathtrace.cu:236-251) a pixel's rays leave a lens -- the eye moved by up to lensRadius 0.8 in
// WORLD x / y -- towards the pixel's focus point pFocus on the plane z = eye.z +- 11.  A point c is on such a ray iff
// c = e + mu (pFocus - e), mu = (c.z - eye.z) / (+-11) > 0, i.e. pFocus = centre(c) + l (1 - 1/mu) with centre(c) the perspective
// image of c on the focus plane and |l| <= 0.8: a disc of radius rho(c) = 0.8 |1 - 1/mu| around it.  Over a box, centre() is a
// projective map (the hull of the corners' images) and rho is extremal at a corner, so the box's focus points lie within the corners'
// images widened by the LARGEST corner radius; each is then projected to pixels through the pinhole (the relation between a pixel and
// its focus point) at the four corners of its bounding square.  Anything doubtful -- a corner not in front of the lens plane, a frame
// whose pixels do not all look towards the same side of it -- keeps the whole frame.
// (pure host arithmetic: ptx_debug_tile_geoms hands it to the CPU tests, which check the superset property ray by ray)
void tile_geom_masks(const DCamera &c, int tile_rows, int tile_rank, int tile_world, int owned, int maxTiles, int ngeoms, const float *aabb8,
                     bool dof, std::vector<uint32_t> &masks) {
    const int W = c.resx, H = c.resy;
    // p - eye = l * (view - R sx - U sy),  R = right * pixelLength.x, U = up * pixelLength.y,  sx = x - W/2, sy = y - H/2  (generateRay)
    const double V[3] = {c.view[0], c.view[1], c.view[2]};
    const double R[3] = {(double)c.right[0] * c.pixelLength[0], (double)c.right[1] * c.pixelLength[0], (double)c.right[2] * c.pixelLength[0]};
    const double U[3] = {(double)c.up[0] * c.pixelLength[1], (double)c.up[1] * c.pixelLength[1], (double)c.up[2] * c.pixelLength[1]};
    // solve [V  -R  -U] (l, l sx, l sy)^T = p - eye by Cramer's rule
    auto det3 = [](const double *a, const double *b, const double *d) {
        return a[0] * (b[1] * d[2] - b[2] * d[1]) - b[0] * (a[1] * d[2] - a[2] * d[1]) + d[0] * (a[1] * b[2] - a[2] * b[1]);
    };
    const double nR[3] = {-R[0], -R[1], -R[2]}, nU[3] = {-U[0], -U[1], -U[2]};
    const double D = det3(V, nR, nU);
    // pixel coordinates of the point eye + p; false: not safely in front of the eye
    auto project = [&](const double p[3], double &x, double &y) {
        const double l = det3(p, nR, nU) / D, lsx = det3(V, p, nU) / D, lsy = det3(V, nR, p) / D;
        // in front of the eye by a margin relative to the point's distance (|view| = 1): otherwise the projection is meaningless
        if (!(l > 1e-6 * (std::fabs(p[0]) + std::fabs(p[1]) + std::fabs(p[2])) && l > 1e-12)) return false;
        x = lsx / l + W * 0.5; y = lsy / l + H * 0.5;
        return std::isfinite(x) && std::isfinite(y);
    };
    double zsign = 0.0;                                      // depth of field: the side of the lens plane every pixel looks to
    bool dof_ok = true;
    if (dof) {
        for (int k = 0; k < 4; k++) {                        // the frame's corner pixels (+- the jitter): z of the unnormalised direction
            const double sx = ((k & 1) ? W + 1.0 : -1.0) - W * 0.5, sy = ((k & 2) ? H + 1.0 : -1.0) - H * 0.5;
            const double dx = V[0] - R[0] * sx - U[0] * sy, dy = V[1] - R[1] * sx - U[1] * sy, dz = V[2] - R[2] * sx - U[2] * sy;
            const double z = dz / std::sqrt(dx * dx + dy * dy + dz * dz);
            if (!(std::fabs(z) > 0.05) || (zsign != 0.0 && (z > 0) != (zsign > 0))) dof_ok = false;
            zsign = z > 0 ? 1.0 : -1.0;
        }
    }
    std::vector<int> rect((size_t)ngeoms * 4);
    for (int g = 0; g < ngeoms; g++) {
        int *r = &rect[(size_t)g * 4];
        r[0] = 0; r[1] = W - 1; r[2] = 0; r[3] = H - 1;                  // x0, x1, y0, y1: the whole frame unless proven smaller
        const float *b = aabb8 + (size_t)g * 8;
        bool ok = std::isfinite(D) && std::fabs(D) > 1e-30 && dof_ok;
        double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
        double cp[8][3], rho = 0.0;
        for (int k = 0; k < 8 && ok; k++) {
            cp[k][0] = (double)((k & 1) ? b[4] : b[0]) - c.position[0]; cp[k][1] = (double)((k & 2) ? b[5] : b[1]) - c.position[1];
            cp[k][2] = (double)((k & 4) ? b[6] : b[2]) - c.position[2];
            if (!std::isfinite(cp[k][0]) || !std::isfinite(cp[k][1]) || !std::isfinite(cp[k][2])) ok = false;
            if (ok && dof) {
                const double mu = cp[k][2] / (zsign * 11.0);             // focalDistance 11 (src/pathtrace.cu:238)
                if (!(mu > 1e-3)) { ok = false; break; }                 // not in front of the lens plane: no bound from this corner
                rho = std::max(rho, 0.8 * std::fabs(1.0 - 1.0 / mu) * 1.0001 + 1e-6);      // lensRadius .8 (:237)
            }
        }
        for (int k = 0; k < 8 && ok; k++) {
            if (!dof) {
                double x, y;
                if (!project(cp[k], x, y)) { ok = false; break; }
                xlo = std::min(xlo, x); xhi = std::max(xhi, x); ylo = std::min(ylo, y); yhi = std::max(yhi, y);
                continue;
            }
            const double mu = cp[k][2] / (zsign * 11.0);
            const double fx = cp[k][0] / mu, fy = cp[k][1] / mu;         // the corner's image on the focus plane (relative to the eye)
            for (int q = 0; q < 4 && ok; q++) {
                const double p[3] = {fx + ((q & 1) ? rho : -rho), fy + ((q & 2) ? rho : -rho), zsign * 11.0};
                double x, y;
                if (!project(p, x, y)) { ok = false; break; }
                xlo = std::min(xlo, x); xhi = std::max(xhi, x); ylo = std::min(ylo, y); yhi = std::max(yhi, y);
            }
        }
        if (!ok || !(xlo <= xhi) || !(ylo <= yhi)) continue;
        // a pixel's rays cover [x - 0.5, x + 0.5] (antialiasing jitter, generateRay); two more pixels for the fp32 ray arithmetic
        const double m = 2.5;
        r[0] = (int)std::max(0.0, std::min((double)W, std::floor(xlo - m)));
        r[1] = (int)std::max(-1.0, std::min((double)W - 1, std::ceil(xhi + m)));
        r[2] = (int)std::max(0.0, std::min((double)H, std::floor(ylo - m)));
        r[3] = (int)std::max(-1.0, std::min((double)H - 1, std::ceil(yhi + m)));
    }
    masks.assign((size_t)maxTiles, 0u);
    auto owned_xy = [&](int i, int &x, int &y) {                        // = owned_pixel (device)
        const int r = i / W;
        x = i - r * W;
        if (tile_world <= 1) { y = r; return; }
        const int k = r / tile_rows;
        y = (k * tile_world + tile_rank) * tile_rows + (r - k * tile_rows);
    };
    for (int tile = 0; tile < maxTiles; tile++) {
        const int i0 = tile * TILE, i1 = std::min(i0 + TILE, owned) - 1;
        if (i1 < i0) { masks[tile] = 0xffffffffu; continue; }
        int x0, y0, x1, y1;
        owned_xy(i0, x0, y0); owned_xy(i1, x1, y1);
        if (y0 != y1) { x0 = 0; x1 = W - 1; }                            // wraps: whole rows y0 .. y1 (rows of other ranks in between included)
        uint32_t m = 0;
        for (int g = 0; g < ngeoms; g++) {
            const int *r = &rect[(size_t)g * 4];
            if (!(r[1] < x0 || r[0] > x1 || r[3] < y0 || r[2] > y1)) m |= 1u << g;
        }
        masks[tile] = m;
    }
}

int owned_pixels(int W, int H, int tile_rows, int tile_rank, int tile_world) {
    int rows = 0;
    for (int y = 0; y < H; y++) if (tile_world <= 1 || (y / tile_rows) % tile_world == tile_rank) rows++;
    return rows * W;
}

std::vector<float> triangle_table(const float *faces15, int nfaces) {
    std::vector<float> tri9((size_t)std::max(nfaces, 1) * 9, 0.f);
    for (int j = 0; j < nfaces; j++) {
        const float *f = faces15 + (size_t)j * 15;
        float *o = &tri9[(size_t)j * 9];
        for (int k = 0; k < 3; k++) { o[k] = f[k]; o[3 + k] = f[5 + k] - f[k]; o[6 + k] = f[10 + k] - f[k]; }
    }
    return tri9;
}

// The geoms a path can end on WITH radiance: bit g = geom g's material emits (emittance > 0, classifyPath's test of the hit's material).
// The last bounce of a launch set looks only for these (k_bounce's light-only variant).  (A material index outside the table sets no bit; geoms beyond
// 31 have none -- such scenes do not take the tile path.)
uint32_t light_geom_bits(int nmaterials, const DMaterial *mats, int ngeoms, const int32_t *geom_material) {
    uint32_t bits = 0;
    for (int g = 0; g < ngeoms && g < 32; g++) {
        const int m = geom_material[g];
        if (m >= 0 && m < nmaterials && mats[m].emittance > 0.0f) bits |= 1u << g;
    }
    return bits;
}

// The object-space box of a small mesh for the candidate pre-test (cullMask / objBoxReach in pt_device.h, which describes the table).
// M, tau: the 3 x 3 part and the translation of the geom's inverse transform (the matrix the exact test maps the ray with), c, half: centre
// and half extent of the faces' vertices in that space, R = |half|_2, cw = fl(M^-1 (c - tau)) the world point stored for the centre,
// rho = (c - tau) - M cw what its rounding leaves (computed here, in binary64).  u = 2^-24.
//
// THE MARGINS, DERIVED.  For a world ray (o, d), |d| = 1, write q* = M o + tau - c and e* = M d for its exact image relative to the
// centre.  A ray the exact test accepts a face for must pass objBoxReach.  Four things stand between the two:
//  (1) the reference's triangle test in binary32 accepts rays that pass within 64 u (D + L) / kappa of the triangle or start that far
//      beyond it (pt_bvh.h derives this; D <= |q*| + R the origin's distance, L <= 2R the longest edge, kappa the triangle's conditioning)
//      = 2^11 u (|q*| + 3R) for kappa >= 2^-5 -- bvhSlack's constant, with the same caveat: below that conditioning the reference
//      decides by rounding noise, and equality is measured (tests/test_cull_objboxes.py, tests/test_gpu_objbox_cull.py), not proven;
//  (2) the reference maps the ray itself in binary32 (mulRows, three roundings deep; normalize): its origin is off by
//      3.1 u (|M||o| + |tau|)_i <= 3.1 u (KA (|q*| + |rho|) + (|M||cw|)_i + |tau_i|) and its direction by an angle of (3.1 KB + 3) u, which
//      moves a point of the box by that times its distance from the origin, at most |q*| + 2R;
//      KA = || |M| |M^-1| ||_inf and KB = max_i |row_i(M)|_2 |M^-1|_F are the two condition numbers that occur (a rotation with a uniform
//      scale: KA <= 3, KB <= 1.8);
//  (3) the pre-test's own q and e: p = fl(o - cw), then a product and two fused multiply-adds per component:
//      |q - q*|_i <= 4.1 u KA (|q*| + |rho|) + |rho_i|,  |e - e*|_i <= 3.1 u |row_i|_2.  The computed pair is the exact image of a ray moved
//      by that much; a point of the box at parameter t <= (|q*| + 2R) / |e*| moves by |q - q*| + t |e - e*| <= ... + 3.2 u KB (|q*| + 2R);
//  (4) the six comparisons.  The box axes compare without rounding.  A cross axis rounds two products and two multiply-adds on each
//      side: |L| <= |l| (1 + u) + 1.01 u |q_k e_j| + 2 eta and R >= r (1 - 2u) - 2 eta + 2^-100 (eta <= 2^-126: underflow), so a half extent
//      larger by 8 u (h_i + |q|_inf) per axis decides every |l| <= r as not separated; h = H + k |q|_1 itself loses 4 u of its value
//      to its three additions and one product, inside the 8.
// Sum, per axis i, with |q*|_inf <= |q*|_2 <= |q*|_1 <= (1 + 13 u KA) |q|_1 + 3 |rho|:
//      margin_i <= u (2^11 + 7.2 KA + 6.3 KB + 11) |q|_1  +  u (3 * 2^11 + 13 KB + 14) R  +  3.1 u ((|M||cw|)_i + |tau_i|) + (1 + 8 u KA) |rho|_inf.
// The table holds  k = u W / (1 - 32 u (KA + KB)),  W = 2^11 + 8 KA + 7 KB + 12  (the divisor pays for the second-order terms: the margins'
// own contribution to "2R", |q*| against the computed |q|), and  H_i = half_i + 4 k R + 4 u ((|M||cw|)_i + |tau_i|) + 2 |rho|_inf,  rounded
// up: the form of bvhSlack (2^11 u (|o - c| + 4R)) with the matrix's conditioning added.  A FLAT mesh has half_i = 0 on an axis and still
// H_i >= 4 k R > 0.  There is no term for the origin's size: o enters through o - cw only, so CULL_FAR_ORIGIN does not occur; rays
// from beyond it keep every candidate as before (cull == 2).  No entry (the world box goes on deciding) for a geom without faces, a
// matrix that is singular, not finite or conditioned worse than 2^16, or a box outside [2^-60, 2^60]: the derivation assumes none of them.
bool objcull_entry(const float *inverse16, const float *faces15, int nfaces, double margin, float out16[OBJCULL_WORDS]) {
    for (int k = 0; k < OBJCULL_WORDS; k++) out16[k] = 0.f;
    if (!inverse16 || !faces15 || nfaces < 1) return false;
    double M[3][3], tau[3], lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) M[r][c] = inverse16[c * 4 + r]; tau[r] = inverse16[12 + r]; }
    for (int j = 0; j < nfaces; j++)
        for (int v = 0; v < 3; v++)
            for (int r = 0; r < 3; r++) {
                const double x = faces15[(size_t)j * 15 + v * 5 + r];
                if (!std::isfinite(x)) return false;
                lo[r] = std::min(lo[r], x); hi[r] = std::max(hi[r], x);
            }
    double I[3][3];                                  // M^-1 by cofactors
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    if (!std::isfinite(det) || det == 0.0) return false;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            I[r][c] = (M[r1][c1] * M[r2][c2] - M[r1][c2] * M[r2][c1]) / det;
        }
    double KA = 0.0, KB = 0.0, fro = 0.0;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) fro += I[r][c] * I[r][c];
    fro = std::sqrt(fro);
    for (int r = 0; r < 3; r++) {
        double sum = 0.0;
        for (int c = 0; c < 3; c++) for (int m = 0; m < 3; m++) sum += std::fabs(M[r][m]) * std::fabs(I[m][c]);
        KA = std::max(KA, sum);
        KB = std::max(KB, std::sqrt(M[r][0] * M[r][0] + M[r][1] * M[r][1] + M[r][2] * M[r][2]) * fro);
    }
    if (!(KA <= 65536.0 && KB <= 65536.0)) return false;
    const double u = 1.0 / 16777216.0;
    double c[3], half[3], R = 0.0, rho = 0.0;
    float cw[3];
    for (int r = 0; r < 3; r++) { c[r] = 0.5 * (lo[r] + hi[r]); half[r] = std::max(hi[r] - c[r], c[r] - lo[r]); R += half[r] * half[r]; }
    R = std::sqrt(R);
    for (int r = 0; r < 3; r++) cw[r] = (float)(I[r][0] * (c[0] - tau[0]) + I[r][1] * (c[1] - tau[1]) + I[r][2] * (c[2] - tau[2]));
    for (int r = 0; r < 3; r++) rho = std::max(rho, std::fabs((c[r] - tau[r]) - (M[r][0] * cw[0] + M[r][1] * cw[1] + M[r][2] * cw[2])));
    const double k = margin * u * (2048.0 + 8.0 * KA + 7.0 * KB + 12.0) / (1.0 - 32.0 * u * (KA + KB));
    for (int r = 0; r < 3; r++) {
        const double mcw = std::fabs(M[r][0] * cw[0]) + std::fabs(M[r][1] * cw[1]) + std::fabs(M[r][2] * cw[2]);
        // (rho is kept at any margin: it is where the stored centre IS, not a bound on rounding; 1e-300 instead of 0 for margin = 0 on a flat axis
        // would be a margin too, so there H_i may be 0)
        const double H = half[r] + 4.0 * k * R + margin * 4.0 * u * (mcw + std::fabs(tau[r])) + 2.0 * rho;
        if (!std::isfinite(H) || H > 0x1p60 || (margin > 0.0 && H < 0x1p-60) || !(std::fabs((double)cw[r]) <= 0x1p60)) { for (int q = 0; q < OBJCULL_WORDS; q++) out16[q] = 0.f; return false; }
        out16[r * 4 + 0] = (float)M[r][0]; out16[r * 4 + 1] = (float)M[r][1]; out16[r * 4 + 2] = (float)M[r][2]; out16[r * 4 + 3] = cw[r];
        out16[12 + r] = margin > 0.0 ? nextafterf((float)H, INFINITY) : (float)H;
    }
    out16[15] = margin > 0.0 ? nextafterf((float)k, INFINITY) : 0.f;
    return true;
}

void cube_face_tables(const float *invT_rows12, float *cnorm18, float *ctan36) {
    for (int side = 0; side < 6; side++) {
        const int axis = side >> 1;
        const float sgn = (side & 1) ? 1.f : -1.f;
        const vec3 e = V3(axis == 0 ? sgn : 0.f, axis == 1 ? sgn : 0.f, axis == 2 ? sgn : 0.f);
        const vec3 n = normalize(mulRows(invT_rows12, e, 0.0f));
        float *o = cnorm18 + side * 3;
        o[0] = n.x; o[1] = n.y; o[2] = n.z;
        vec3 perp1, perp2;
        tangentFrame(V3(o[0], o[1], o[2]), perp1, perp2);      // (of the floats the kernels read back as the normal)
        float *t = ctan36 + side * 6;
        t[0] = perp1.x; t[1] = perp1.y; t[2] = perp1.z; t[3] = perp2.x; t[4] = perp2.y; t[5] = perp2.z;
    }
}

// scene upload (pathtraceInit, src/pathtrace.cu:111-146) -- flattened, no host struct is mutated
int pt_prepare_scene(int ngeoms, const ptx_geom *geoms, int nmaterials, const ptx_material *materials, const ptx_options &opt, int owned,
                     int nbins, size_t lds_limit, const SceneSwitches &sw, HostScene &hs) {
    hs = HostScene();
    const size_t ng1 = (size_t)std::max(ngeoms, 1);
    hs.geoms.resize(ng1);
    for (int i = 0; i < ngeoms; i++) {
        const ptx_geom &g = geoms[i];
        DGeom &d = hs.geoms[i];
        memset(&d, 0, sizeof d);
        memcpy(d.xf, g.transform, 64); memcpy(d.inv, g.inverseTransform, 64); memcpy(d.invT, g.invTranspose, 64);
        d.type = g.type; d.materialid = g.materialid;
        d.faceStart = (int32_t)(hs.faces.size() / 15); d.faceCount = g.faceSize;
        if (g.faceSize) hs.faces.insert(hs.faces.end(), g.faces, g.faces + (size_t)g.faceSize * 15);
        const ptx_texture *tx[4] = {&g.kd, &g.ks, &g.ke, &g.bump};
        for (int k = 0; k < 4; k++) {
            DTex &dt = d.tex[k];
            if (tx[k]->channels > 0 && tx[k]->image && tx[k]->width > 0 && tx[k]->height > 0) {
                if (tx[k]->channels < 3) return set_error(PTX_ERR_UNSUPPORTED, "textures need >= 3 channels");
                dt.w = tx[k]->width; dt.h = tx[k]->height; dt.ch = tx[k]->channels; dt.off = hs.texels.size();
                hs.uses_uv = 1;
                size_t nbytes = (size_t)dt.w * dt.h * dt.ch;
                hs.texels.insert(hs.texels.end(), tx[k]->image, tx[k]->image + nbytes);
            }
        }
    }
    hs.ntri = (int)(hs.faces.size() / 15);
    hs.tri9 = triangle_table(hs.faces.data(), hs.ntri);
    // a BVH for every mesh with enough faces to repay it (pt_bvh.h); its nodes and leaf triangles stay in global memory
    hs.roots.assign(ng1, -1); hs.depths.assign(ng1, 0); hs.wroots.assign(ng1, -1); hs.wneeds.assign(ng1, 0);
    for (int i = 0; i < ngeoms; i++)
        if (hs.geoms[i].type == G_OBJ && hs.geoms[i].faceCount >= BVH_MIN_FACES && !opt.no_bvh) {
            hs.roots[i] = bvhBuild(hs.faces.data(), hs.tri9.data(), hs.geoms[i].faceStart, hs.geoms[i].faceCount, hs.bvh, &hs.depths[i], &hs.wroots[i], &hs.wneeds[i]);
            if (sw.no_wide_bvh) hs.wroots[i] = -1;
            hs.bvh_meshes++;
        }
    hs.bvh_nodes = (int)(hs.bvh.nodes.size() / 2);
    if (sw.no_wide_bvh) hs.bvh.wide.clear();
    {   // stack entries per lane for k_mesh: deepest tree + 1 (a tree of depth d needs d + 1), at least 8, at most BVH_STACK
        int deepest = 0;
        // (a tree walks its four-wide nodes when their walk fits BVH_STACK entries, else the binary tree front to back when
        // that fits, else the skip links: the stack is as long as the longest walk that is taken)
        for (int i = 0; i < ngeoms; i++) {
            if (hs.roots[i] < 0) continue;
            if (hs.wroots[i] >= 0 && hs.wneeds[i] <= BVH_STACK) deepest = std::max(deepest, hs.wneeds[i] - 1);
            else if (hs.depths[i] < BVH_STACK) deepest = std::max(deepest, hs.depths[i]);
        }
        hs.bvh_stack = std::min(BVH_STACK, std::max(8, deepest + 1));
    }
    if (!hs.bvh_meshes && !sw.no_chunks)          // spread the loops of small meshes over lanes (tileIntersect)
        for (int i = 0; i < ngeoms; i++)
            if (hs.geoms[i].type == G_OBJ) hs.mesh_chunks = std::max(hs.mesh_chunks, (hs.geoms[i].faceCount + MESH_CHUNK - 1) / MESH_CHUNK);
    // materials and geom tables go to LDS; the triangle tables join them when that leaves room for at least 2 workgroups
    // per CU (160 KB LDS, ~19 KB of sort buffers) -- otherwise they are read from global memory (L2-resident)
    hs.tri_lds = (((size_t)nmaterials * 11 + (size_t)ngeoms * 58) * 4 <= 56 * 1024 && !opt.no_lds_triangles) ? 1 : 0;
    hs.ntri_lds = (hs.tri_lds && ((size_t)hs.ntri * 27 + (size_t)nmaterials * 11 + (size_t)ngeoms * 58) * 4 <= 56 * 1024) ? hs.ntri : 0;
    {   // k_bounce's dynamic LDS grows with the scene (tables) and with the number of material bins (ranking histogram):
        // check it against the device limit here, where the caller can be told, not at the first launch.  Step down first
        // (triangle tables, then all tables, to global memory: the plain per-ray loop over the geoms takes over), refuse
        // only what cannot run at all.
        auto need = [&]() { return sizeof(int32_t) * (bounceLdsWords(hs.tri_lds ? sceneTableWords(hs.ntri_lds, nmaterials, ngeoms) : 0, nbins) + QUEUE_WORDS); };
        if (need() > lds_limit && hs.ntri_lds) hs.ntri_lds = 0;
        if (need() > lds_limit && hs.tri_lds) hs.tri_lds = 0;
        if (need() > lds_limit)
            return set_error(PTX_ERR_UNSUPPORTED, "material sort over " + std::to_string(nbins) + " materials needs " + std::to_string(need()) +
                             " bytes of LDS per workgroup, the device offers " + std::to_string(lds_limit) + ": render with sort_by_material = 0 (same image "
                             "only if the reference is built with SORT_BY_MATERIAL 0 too)");
    }
    // per-geom table for the per-lane gathers (rows 0-2 of the three matrices) and conservative world boxes
    hs.gtab.assign(ng1 * GTAB_WORDS, 0.f); hs.aabb.assign(ng1 * 8, 0.f);
    for (int i = 0; i < ngeoms; i++) {
        const DGeom &d = hs.geoms[i];
        float *o = &hs.gtab[(size_t)i * GTAB_WORDS];
        const float *mats3[3] = {d.inv, d.xf, d.invT};
        for (int m = 0; m < 3; m++)
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) o[m * 12 + r * 4 + c] = mats3[m][c * 4 + r];
        int32_t ints[4] = {d.type, d.materialid, d.faceStart, d.faceCount};
        memcpy(o + 36, ints, sizeof ints);
        float box[6];
        make_world_aabb(d, hs.faces, box);
        for (int k = 0; k < 3; k++) { hs.aabb[(size_t)i * 8 + k] = box[k]; hs.aabb[(size_t)i * 8 + 4 + k] = box[3 + k]; }
        if (i < 32) {
            if (d.type == G_OBJ) hs.mesh_bits |= 1u << i;
            else if (d.type == G_CUBE) hs.cube_bits |= 1u << i;
            else if (d.type == G_SPHERE) hs.sphere_bits |= 1u << i;
        }
    }
    // (the device reads the boxes as centre + half extent; the host keeps corners for the camera tile masks)
    hs.aabb_ch.assign(hs.aabb.size(), 0.f);
    for (int i = 0; i < ngeoms; i++) world_box_centre_half(&hs.aabb[(size_t)i * 8], &hs.aabb_ch[(size_t)i * 8]);
    hs.cull = (hs.tri_lds && ngeoms >= 1 && ngeoms <= 32 && !opt.no_cull) ? 1 : 0;
    // 2: some world box reaches beyond CULL_FAR_ORIGIN / 2 (or is unbounded: a NaN vertex), so rays can START that far out -- the
    // candidate pre-test then looks at every ray's origin (cullMask, pt_device.h: FAR ORIGINS)
    for (int i = 0; i < ngeoms && hs.cull; i++)
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(hs.aabb[(size_t)i * 8 + k]) <= 0.5f * CULL_FAR_ORIGIN && std::fabs(hs.aabb[(size_t)i * 8 + 4 + k]) <= 0.5f * CULL_FAR_ORIGIN)) hs.cull = 2;
    // object-space boxes for the small meshes that tileIntersect works off as pair-list entries (the scenes mesh_chunks counts: no mesh has a BVH)
    hs.objcull.assign(ng1 * OBJCULL_WORDS, 0.f);
    if (hs.cull && !hs.bvh_meshes && !sw.no_chunks && !sw.no_objcull)
        for (int i = 0; i < ngeoms; i++)
            if (hs.geoms[i].type == G_OBJ && objcull_entry(hs.geoms[i].inv, hs.faces.data() + (size_t)hs.geoms[i].faceStart * 15, hs.geoms[i].faceCount, 1.0, &hs.objcull[(size_t)i * OBJCULL_WORDS]))
                hs.objcull_bits |= 1u << i;
    // normals that do not depend on the ray, computed once with the device's own functions (compiled for the host with
    // the same flags: no contraction, IEEE divide and square root), so the kernels read what they would have computed
    hs.fnorm.assign((size_t)std::max(hs.ntri, 1) * 3, 0.f); hs.cnorm.assign(ng1 * 18, 0.f);
    hs.ctan.assign(ng1 * CTAN_WORDS, 0.f);
    for (int i = 0; i < ngeoms; i++) {
        const DGeom &d = hs.geoms[i];
        if (d.type == G_OBJ) {
            if (d.tex[3].ch && i < 32) hs.bump_bits |= 1u << i;
            for (int j = 0; j < d.faceCount; j++) {          // meshIntersectionTest, src/intersections.h:237-243
                const float *tri = &hs.faces[((size_t)d.faceStart + j) * 15];
                const vec3 e1 = sub(ld3(tri + 5), ld3(tri)), e2 = sub(ld3(tri + 10), ld3(tri));
                const vec3 objN = normalize(cross(e1, e2));
                const vec3 n = normalize(multiplyMV(d.invT, objN, 0.f));
                float *o = &hs.fnorm[((size_t)d.faceStart + j) * 3];
                o[0] = n.x; o[1] = n.y; o[2] = n.z;
            }
        } else if (d.type == G_CUBE) {                       // boxIntersectionTest, src/intersections.h:86
            cube_face_tables(&hs.gtab[(size_t)i * GTAB_WORDS + 24], &hs.cnorm[(size_t)i * 18], &hs.ctan[(size_t)i * CTAN_WORDS]);
        }
    }
    if (ngeoms > 32) hs.bump_bits = 0xffffffffu;          // (no per-geom bit beyond 32 geoms: such scenes do not take the tile path)
    if (hs.faces.empty()) hs.faces.resize(15, 0.f);
    if (hs.texels.empty()) hs.texels.resize(16, 0);
    hs.mats.resize((size_t)std::max(nmaterials, 1));
    static_assert(sizeof(DMaterial) == sizeof(ptx_material), "material layout");
    if (nmaterials) memcpy(hs.mats.data(), materials, sizeof(DMaterial) * (size_t)nmaterials);
    for (const DMaterial &m : hs.mats) hs.h_spec.push_back(m.hasReflective > 0.0f || m.hasRefractive > 0.0f ? 1 : 0);
    {
        std::vector<int32_t> gm((size_t)ngeoms);
        for (int i = 0; i < ngeoms; i++) gm[i] = hs.geoms[i].materialid;
        hs.light_bits = light_geom_bits(nmaterials, hs.mats.data(), ngeoms, gm.data());
    }
    {   // which records carry what (record_masks); off: more than 64 bins, no material, or PTX_DEBUG_NO_DIR_SKIP
        unsigned long long need = ~0ull, cubes = 0ull;
        const bool off = nbins > 64 || nmaterials < 1 || sw.no_dir_skip;
        if (!off) {
            std::vector<int> gt((size_t)ngeoms), gm((size_t)ngeoms);
            for (int i = 0; i < ngeoms; i++) { gt[i] = hs.geoms[i].type; gm[i] = hs.geoms[i].materialid; }
            record_masks(nmaterials, hs.mats.data(), ngeoms, gt.data(), gm.data(), opt.sort_by_material != 0, need, cubes);
        }
        hs.dir_bins = off ? ~0ull : need;
        // (the code rides in bits 28-30 of the pixel slot; the tabulated normals are what the tile path's decodeKey reads)
        hs.ntab_bins = (off || !hs.cull || owned >= (1 << 28) || sw.no_normal_codes) ? 0ull : cubes;
    }
    // split mesh search: worth it when some mesh is big enough for a BVH; needs the candidate masks (cull, <= 32 geoms: a
    // parked ray carries one bit per mesh whose box it reaches) and a queue entry per ray in the worst case
    hs.split_mesh = hs.bvh_meshes > 0 && hs.cull && !opt.no_mesh_split;
    if (sw.force_split) hs.split_mesh = hs.cull && hs.mesh_bits != 0;      // (any scene with a mesh)
    if (hs.tri_lds) {   // the scene tables as k_bounce stages them (split: without the triangle tables), in one array: DScene::ldsblob
        const size_t nl = hs.split_mesh ? 0 : (size_t)hs.ntri_lds;
        const float *m = reinterpret_cast<const float *>(hs.mats.data());
        auto put = [&](const float *src, size_t n) { hs.ldsblob.insert(hs.ldsblob.end(), src, src + n); };
        put(hs.tri9.data(), nl * 9); put(hs.faces.data(), nl * 15); put(m, (size_t)nmaterials * 11);
        put(hs.gtab.data(), (size_t)ngeoms * GTAB_WORDS); put(hs.fnorm.data(), nl * 3); put(hs.cnorm.data(), (size_t)ngeoms * 18);
    }
    return PTX_OK;
}

}  // namespace ptd

extern "C" {

// CPU-only check of the mesh BVH: builds the tree of `nfaces` faces and searches `nrays` object-space rays (origin,
// direction; the direction is normalised the way meshIntersectionTest does) with the tree and with the plain loop.
static int64_t g_bvh_visits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
int ptx_debug_bvh_check(const float *faces15, int nfaces, const float *rays6, int nrays, int32_t *face_loop, float *t_loop,
                        int32_t *face_bvh, float *t_bvh, int64_t *stats4) {
    if (!faces15 || !rays6 || !face_loop || !t_loop || !face_bvh || !t_bvh || nfaces < 1 || nrays < 0)
        return set_error(PTX_ERR_INVALID, "ptx_debug_bvh_check: bad argument");
    const std::vector<float> tri9 = triangle_table(faces15, nfaces);
    BvhBuild bb;
    int depth = 0;
    int wroot = -1, wneed = 0;
    const int root = bvhBuild(faces15, tri9.data(), 0, nfaces, bb, &depth, &wroot, &wneed);
    std::vector<int32_t> wstack((size_t)std::max(wneed, 1) + 1, 0x7fffffff);      // (+ a guard word: the walk must never reach it)
    long long visited = 0, visited_ordered = 0, visited_wide = 0, mismatches = 0, group_max = 0, sum_group_max = 0, groups = 0, tris_wide = 0;
    for (int i = 0; i < nrays; i++) {
        const vec3 o = V3(rays6[i * 6 + 0], rays6[i * 6 + 1], rays6[i * 6 + 2]);
        const vec3 d = normalize(V3(rays6[i * 6 + 3], rays6[i * 6 + 4], rays6[i * 6 + 5]));
        int f0, f1, vis = 0;
        float b0, b1;
        t_loop[i] = loopNearestHost(faces15, tri9.data(), nfaces, o, d, f0);
        t_bvh[i] = bvhNearest(bb.nodes.data(), bb.tris.data(), root, o, d, f1, b0, b1, &vis);
        if (depth < BVH_STACK) {                // the front-to-back search must agree with the skip-link one
            int f2, vis2 = 0;
            float c0, c1;
            int32_t stack[BVH_STACK];
            const float t2 = bvhNearestOrdered(bb.nodes.data(), bb.tris.data(), root, o, d, f2, c0, c1, stack, 1, &vis2);
            visited_ordered += vis2;
            if (f2 != f1 || memcmp(&t2, &t_bvh[i], 4) != 0 || (f1 >= 0 && (memcmp(&c0, &b0, 4) != 0 || memcmp(&c1, &b1, 4) != 0))) mismatches++;
        }
        if (wroot >= 0) {                       // ... and so must the walk over the four-wide nodes
            int f3, vis3 = 0;
            float e0, e1;
            const float t3 = bvhNearestWide(bb.nodes.data(), bb.wide.data(), bb.tris.data(), root, wroot, o, d, f3, e0, e1, wstack.data(), 1, &vis3);
            visited_wide += vis3 & 0xffff;
            tris_wide += vis3 >> 16;
            group_max = std::max(group_max, (long long)(vis3 & 0xffff) / 4);
            if (i % 64 == 63 || i == nrays - 1) { sum_group_max += group_max; group_max = 0; groups++; }
            if (wstack[(size_t)std::max(wneed, 1)] != 0x7fffffff) mismatches += 1000000;      // the walk overran the stack bound the builder computed
            if (f3 != f1 || memcmp(&t3, &t_bvh[i], 4) != 0 || (f1 >= 0 && (memcmp(&e0, &b0, 4) != 0 || memcmp(&e1, &b1, 4) != 0))) mismatches++;
            {   // the same steps under the schedule of k_mesh's refilling waves: one node or ONE triangle per turn
                WideWalk w;
                wideStart(w, bb.nodes[2 * (size_t)root], bb.nodes[2 * (size_t)root + 1], wroot, o, d);
                while (w.n != WIDE_DONE) {
                    if (w.n >= 0) wideNodeStep(w, bb.wide.data(), wstack.data(), 1);
                    else wideLeafStep<true>(w, bb.tris.data(), wstack.data(), 1);
                }
                if (wstack[(size_t)std::max(wneed, 1)] != 0x7fffffff) mismatches += 1000000;
                if (w.face != f1 || memcmp(&w.tmin, &t_bvh[i], 4) != 0 || (f1 >= 0 && (memcmp(&w.b0, &b0, 4) != 0 || memcmp(&w.b1, &b1, 4) != 0))) mismatches++;
            }
        }
        face_loop[i] = f0; face_bvh[i] = f1;
        visited += vis;
    }
    if (stats4) { stats4[0] = (int64_t)(bb.nodes.size() / 2); stats4[1] = (int64_t)(bb.tris.size() / BVH_TRI); stats4[2] = visited; stats4[3] = mismatches; }
    g_bvh_visits[0] = visited; g_bvh_visits[1] = visited_ordered; g_bvh_visits[2] = visited_wide / 4; g_bvh_visits[3] = wneed;
    g_bvh_visits[4] = sum_group_max; g_bvh_visits[5] = groups; g_bvh_visits[6] = tris_wide; g_bvh_visits[7] = depth;
    return PTX_OK;
}

// CPU-only: ptx_create's rule for what a stored path's record carries (record_masks), for nmaterials <= 64 materials and ngeoms geoms
// given by type and material: masks[0] = dir_bins, masks[1] = ntab_bins (before the conditions of a particular tracer: candidate masks
// on, fewer than 2^28 owned pixels).
int ptx_debug_record_masks(int nmaterials, const ptx_material *materials, int ngeoms, const int32_t *geom_type, const int32_t *geom_material,
                           int sort_by_material, uint64_t masks[2]) {
    if (nmaterials < 1 || nmaterials > 64 || !materials || ngeoms < 0 || (ngeoms && (!geom_type || !geom_material)) || !masks)
    { set_error(PTX_ERR_INVALID, "ptx_debug_record_masks: bad argument"); return -1; }
    unsigned long long d = 0, n = 0;
    record_masks(nmaterials, reinterpret_cast<const DMaterial *>(materials), ngeoms, geom_type, geom_material, sort_by_material != 0, d, n);
    masks[0] = d; masks[1] = n;
    return 0;
}

// CPU-only: ptx_create's light_bits (light_geom_bits) for ngeoms geoms given by their material: bit g = geom g can end a path with radiance.
int ptx_debug_light_bits(int nmaterials, const ptx_material *materials, int ngeoms, const int32_t *geom_material, uint32_t *bits_out) {
    if (nmaterials < 0 || (nmaterials && !materials) || ngeoms < 0 || (ngeoms && !geom_material) || !bits_out)
    { set_error(PTX_ERR_INVALID, "ptx_debug_light_bits: bad argument"); return -1; }
    *bits_out = light_geom_bits(nmaterials, reinterpret_cast<const DMaterial *>(materials), ngeoms, geom_material);
    return 0;
}

// CPU-only: the candidate pre-test's table (world_box_centre_half) for n corner boxes (lo xyz, hi xyz): 8 floats each = centre xyz, 0,
// half extent xyz, 0 -- what cullMask reads on the device.
int ptx_debug_cull_boxes(int n, const float *boxes6, float *centre_half8) {
    if (n < 0 || (n && (!boxes6 || !centre_half8))) { set_error(PTX_ERR_INVALID, "ptx_debug_cull_boxes: bad argument"); return -1; }
    for (int g = 0; g < n; g++) {
        const float lohi[8] = {boxes6[g * 6], boxes6[g * 6 + 1], boxes6[g * 6 + 2], 0.f, boxes6[g * 6 + 3], boxes6[g * 6 + 4], boxes6[g * 6 + 5], 0.f};
        world_box_centre_half(lohi, centre_half8 + (size_t)g * 8);
    }
    return n;
}

// CPU-only: ptx_create's object-space boxes of the small meshes (objcull_entry, the rule of pt_prepare_scene: candidate masks on, no mesh
// with a BVH; no_bvh = ptx_options.no_bvh: no mesh gets one) for ngeoms <= 32 geoms given as ptx_create takes them: table16 = OBJCULL_WORDS
// floats per geom as cullMask reads them on the device, *bits_out = DScene::objcull_bits.  margin 1 = the derived margins, 0 = none (tests only).
int ptx_debug_cull_objboxes(int ngeoms, const ptx_geom *geoms, int no_bvh, float margin, float *table16, uint32_t *bits_out) {
    if (ngeoms < 0 || ngeoms > 32 || (ngeoms && (!geoms || !table16)) || !bits_out || !(margin >= 0.f))
    { set_error(PTX_ERR_INVALID, "ptx_debug_cull_objboxes: bad argument"); return -1; }
    bool bvh = false;
    for (int g = 0; g < ngeoms; g++) {
        if (geoms[g].faceSize < 0 || (geoms[g].faceSize && !geoms[g].faces)) { set_error(PTX_ERR_INVALID, "ptx_debug_cull_objboxes: bad argument"); return -1; }
        bvh = bvh || (!no_bvh && geoms[g].type == G_OBJ && geoms[g].faceSize >= BVH_MIN_FACES);
    }
    *bits_out = 0;
    for (int g = 0; g < ngeoms; g++) {
        for (int k = 0; k < OBJCULL_WORDS; k++) table16[(size_t)g * OBJCULL_WORDS + k] = 0.f;
        if (!bvh && geoms[g].type == G_OBJ && objcull_entry(geoms[g].inverseTransform, geoms[g].faces, geoms[g].faceSize, margin, table16 + (size_t)g * OBJCULL_WORDS))
            *bits_out |= 1u << g;
    }
    return 0;
}

// CPU-only: ptx_create's table of tangent frames (DScene::ctan, cube_face_tables) for ngeoms geoms given as ptx_create takes them:
// out36_per_geom = CTAN_WORDS floats per geom -- side (axis * 2 + (sign > 0)) at side * 6: perp1 xyz, perp2 xyz of that face's tabulated
// normal, as the diffuse sampler would compute them -- zeros for a geom that is not a cube.
int ptx_debug_cube_tangents(int ngeoms, const ptx_geom *geoms, float *out36_per_geom) {
    if (ngeoms < 0 || (ngeoms && (!geoms || !out36_per_geom))) { set_error(PTX_ERR_INVALID, "ptx_debug_cube_tangents: bad argument"); return -1; }
    for (int g = 0; g < ngeoms; g++) {
        float *o = out36_per_geom + (size_t)g * CTAN_WORDS;
        for (int k = 0; k < CTAN_WORDS; k++) o[k] = 0.f;
        if (geoms[g].type != G_CUBE) continue;
        float rows[12], cnorm18[18];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) rows[r * 4 + c] = geoms[g].invTranspose[c * 4 + r];      // (as pt_prepare_scene fills gtab)
        cube_face_tables(rows, cnorm18, o);
    }
    return 0;
}

// CPU-only: the per-tile geom masks of the camera-ray bounce (update_tile_geoms) for a camera, a tile split and a list of world boxes
// (6 floats each: lo xyz, hi xyz), without a tracer or a device.  masks_out[tile], tiles of 256 owned pixels; returns the number of tiles
// (negative: bad argument).
int ptx_debug_tile_geoms(const ptx_camera *camera, int ngeoms, const float *boxes6, int depth_of_field, int tile_rows, int tile_rank, int tile_world,
                         uint32_t *masks_out, int max_tiles) {
    if (!camera || !boxes6 || !masks_out || ngeoms < 1 || ngeoms > 32 || camera->resolution[0] < 1 || camera->resolution[1] < 1)
    { set_error(PTX_ERR_INVALID, "ptx_debug_tile_geoms: bad argument"); return -1; }
    DCamera cam;
    camera_to_device(*camera, cam);
    const int world = tile_world < 1 ? 1 : tile_world, rows = world > 1 ? tile_rows : cam.resy;
    if (world > 1 && (tile_rows < 1 || tile_rank < 0 || tile_rank >= world)) return -1;
    const int owned = owned_pixels(cam.resx, cam.resy, rows, tile_rank, world);
    const int ntiles = (std::max(owned, 1) + TILE - 1) / TILE;
    if (ntiles > max_tiles) return -1;
    std::vector<float> a8((size_t)ngeoms * 8, 0.f);
    for (int g = 0; g < ngeoms; g++)
        for (int k = 0; k < 3; k++) { a8[(size_t)g * 8 + k] = boxes6[g * 6 + k]; a8[(size_t)g * 8 + 4 + k] = boxes6[g * 6 + 3 + k]; }
    std::vector<uint32_t> masks;
    tile_geom_masks(cam, rows, tile_rank, world, owned, ntiles, ngeoms, a8.data(), depth_of_field != 0, masks);
    memcpy(masks_out, masks.data(), sizeof(uint32_t) * (size_t)ntiles);
    return ntiles;
}

// node visits of the last ptx_debug_bvh_check: skip-link walk, front-to-back binary walk, four-wide walk (nodes), wide stack need,
// sum over groups of 64 consecutive rays of the longest four-wide walk in the group, number of groups, triangles the four-wide walk tested,
// depth of the binary tree
int ptx_debug_bvh_visits(int64_t out8[8]) {
    if (!out8) return set_error(PTX_ERR_INVALID, "null argument");
    for (int k = 0; k < 8; k++) out8[k] = g_bvh_visits[k];
    return PTX_OK;
}

}  // extern "C"
