// The tracing megakernel: one launch walks every ray through all elements of the scene.
//
// Reference: Raytracer.trace / sub_trace (raytracer.py:262-415) runs ~25 whole-array NumPy passes per
// surface, each streaming the ray arrays through DRAM.  Here a ray's state (position, direction, weight,
// polarisation, wavelength, current index) lives in registers of one lane for the whole walk; HBM sees only
// the compulsory traffic -- the section stores RayStorage must contain afterwards (ray_storage.py:80-90),
// N*[(M+2)*48+28] bytes with polarisation -- as fully coalesced 512 B / 256 B wavefront stores in the
// reference's struct-of-arrays (Fortran) layout.  Scene constants are wave-uniform scalar loads.
#pragma once
#include "ot_device.hpp"
#include "ot_generate.hpp"

// Event counters (Raytracer._msgs, raytracer.py:289): wave-aggregated (one ballot, the section index is
// wave-uniform) into a per-workgroup LDS table; the persistent workgroup flushes its non-zero entries to the
// global table once at its end.  Global atomics per event would serialise on a handful of hot addresses:
// measured 5.4 ms -> 2.4 ms for the 10 M ray double-Gauss launch when they were removed from the loop.
OT_DEV void count_event(unsigned int* cnt, int nt, int info, int sec, bool cond) {
    unsigned long long m = __ballot(cond);
    if (m != 0ull) {
        int lane = __lane_id();
        if (lane == (int)__ffsll((long long)m) - 1) atomicAdd(&cnt[info * nt + sec], (unsigned int)__popcll(m));
    }
}

struct RayState {
    V3 p, s;
    float w, wl;
    float polx, poly, polz;
    double n_cur;
};

// Raytracer.__compute_polarization raytracer.py:831-879 (hwh == true for this lane).
// Everything in here only reaches float32-stored quantities (pol_list, and through A_ts/A_tp the weight), never
// a position, direction or mask, so it is evaluated with fused multiply-adds and one reciprocal square root
// instead of sqrt + three divisions: agreement with the reference is at the 1e-15 level before the float32
// rounding of the store (bar: 1e-6 relative).
// The reference's PROJECTION form (pol' = A_ts ps + A_tp pp') is kept on purpose: the float32-stored pol is only
// perpendicular to s to ~3e-8, and a rotation form (Rodrigues about ps; 25 % fewer instructions) carries that
// parallel component along instead of dropping it.  That flips the float32 rounding of pol' in ~17 % of the
// components, and since T is first order in pol the weights then drift by ~1e-7 per surface (measured 2.6e-6
// after 15 surfaces) -- outside the 1e-6 bar.
template <bool POL>
OT_DEV void compute_polarization(const V3& s, const V3& s_, const RayState& r, float& npx, float& npy, float& npz,
                                 double& A_ts, double& A_tp) {
#pragma clang fp contract(fast)
    const double inv_sqrt2 = 0.7071067811865475;  // 1/np.sqrt(2)
    if (!POL) {
        A_ts = inv_sqrt2;
        A_tp = inv_sqrt2;
        return;
    }
    bool mask = (s.x != s_.x) || (s.y != s_.y) || (s.z != s_.z);
    V3 ps = cross3(s_, s);
    const double l2 = ps.x * ps.x + ps.y * ps.y + ps.z * ps.z;
    double inv = rsqrt(l2);
    ps.x *= inv;
    ps.y *= inv;
    ps.z *= inv;
    V3 pp = cross3(ps, s);
    V3 pol = {(double)r.polx, (double)r.poly, (double)r.polz};
    A_ts = dot3(ps, pol);
    A_tp = dot3(pp, pol);
    if (!mask) {
        A_ts = inv_sqrt2;
        A_tp = inv_sqrt2;
    }
    V3 pp_ = cross3(ps, s_);
    if (mask) {
        npx = (float)(ps.x * A_ts + pp_.x * A_tp);
        npy = (float)(ps.y * A_ts + pp_.y * A_tp);
        npz = (float)(ps.z * A_ts + pp_.z * A_tp);
    }
    // A small bend (HURB through a wide opening or with small draws, an ideal lens near its centre): s' x s carries
    // ~2^-53 absolute against a length a = |s' x s|, and the part of that error along s tilts ps out of the plane
    // perpendicular to s, so pol' is off by ~2^-53 / a along s (measured 2.7e-3 at a = 2^-48; the reference's own form is
    // as noisy, tests/test_hurb_host.py).  With t the unit vector of s' - s, the projection is exactly
    //     pol' = pol - s (s'.pol) - (1 - cos theta) [t (t.pol) + s (s.pol)],
    // and the last term is below a^2 / 2: under a = 2^-20 the first two are pol' to 2^-41, without any basis.  (At 2^-20
    // the basis form is good to 2^-33: either side of the threshold is far inside the float32 store.)  A_ts and A_tp
    // are not used by the callers that can get here (refract_ideal, hurb_bend: no Fresnel factor).  One comparison on the
    // common path; the rest sits behind a wave-uniform branch that the waves of an ordinary bundle skip (computed for
    // every lane it cost the render-only C5 kernel 2 %).
    const bool small = mask && l2 < 0x1p-40;
    if (__ballot(small) != 0ull) {
        if (small) {
            const double sp = dot3(s_, pol);
            npx = (float)(pol.x - s.x * sp);
            npy = (float)(pol.y - s.y * sp);
            npz = (float)(pol.z - s.z * sp);
        }
    }
}

// |n x s|^2 below which refraction_polarization drops the plane-of-incidence term of pol', i.e. sin(alpha) = 2^-26: where
// the form's rounding error (~3 * 2^-53 / sin(alpha)) meets the size of the dropped term (<= sin(alpha)).  From a host sweep
// of the float64 restatement against exact values (tests/pol_form.py; 2160 rays, sin(alpha) = 2^-30 .. 2^-20, three
// normals, six pairs of media), largest error of pol' before the float32 store in units of the noise part of the bar of
// tests/test_gpu_refraction_step.py (2^-30 + min(2^-25, 2^-49 / sin(alpha))), per threshold:
//     2^-56: 1.47    2^-54: 0.68    2^-53: 0.48    2^-52: 0.46    2^-51: 0.53    2^-50: 0.75    2^-49: 1.10    2^-48: 1.69
// (worst case at 2^-52: sin(alpha) = 2^-25.95 on the flat normal, n = 1.5015 -> 1.5, i.e. the form just above the
// threshold).  The weights use 2e-7 of theirs at every threshold.
#ifndef OT_POL_NEAR
#define OT_POL_NEAR 0x1p-52
#endif

// __compute_polarization and the Fresnel factor for refraction, where s' = N s - q n lies in the plane of n and s.
// With m = n x s (|m| = sin(alpha)) the reference's basis vectors are, by (a x b) x c = b (a.c) - a (b.c):
//     ps  = +-m / |m|                      (the sign cancels in A_ts ps and in A_ts^2)
//     pp  = ps x s  = (ns s - n) / |m|
//     pp' = ps x s' = (W s - (s.s') n) / |m|,      n.s' = W,   s.s' = ct = N - q ns
// so   A_ts = (m.pol)/|m|,  A_tp = tp/|m| with tp = ns (s.pol) - n.pol,  pol' = [(m.pol) m + tp (W s - ct n)] / |m|^2.
// The cross product itself is not needed: {m/|m|, s, e/|m|} with e = n - ns s is an orthonormal frame for unit n and s,
// e.pol = -tp, so the part of pol along m is pol minus its parts along s and e, for ANY pol:
//     (m.pol) m / mm = pol - (s.pol) s + tp e / mm,        (m.pol)^2 / mm = |pol|^2 - (s.pol)^2 - tp^2 / mm,     mm = e.e
//     pol'   = pol - (s.pol) s + (tp / mm) [(W - ns) s + (1 - ct) n]
//     A_tp^2 = tp^2 / mm,       A_ts^2 = P - A_tp^2,       P = |pol|^2 - (s.pol)^2
// No identity relies on pol being exactly perpendicular to s (the float32-stored pol is not; see above why that matters):
// this is the reference's projection to rounding, without a cross product, m.pol or the vector W s - ct n.  mm is e.e,
// which is conditioned like |n x s|^2 and formed from the same n and s as tp, so that tp^2 <= P mm holds to rounding even
// where n is unit only to a few ulps; 1 - ns^2 (three instructions cheaper) has neither property, although the host sweep
// could not tell the two apart by the bars (tests/test_pol_form_host.py).
// The Fresnel factor is closed by refract, which wants the squared amplitudes as A = (A_ts^2 + A_tp^2) M, B = A_tp^2 M
// over a common denominator M: here A = P mm, B = tp^2, M = mm, so that one reciprocal serves T and the 1 / mm of pol'.
// The split between the two amplitudes only enters T through d1^2 - d2^2 = O(sin^2), which cancels its conditioning.
// The products are fused by hand: the file is compiled without contraction, and a pragma does not reach into helpers
// defined elsewhere (dot3 and cross3 of ot_device.hpp came out unfused under `fp contract(fast)`).
// Returns whether pol changes: then pol' = pol - sp s + (tp / M) [...], which refract forms once it has 1 / M.
OT_DEV bool refraction_polarization(const V3& n, const V3& s, const V3& s_, double ns, const RayState& r, double& A,
                                    double& B, double& M, double& tp, double& sp) {
    const V3 pol = {(double)r.polx, (double)r.poly, (double)r.polz};
    sp = __builtin_fma(s.z, pol.z, __builtin_fma(s.y, pol.y, s.x * pol.x));
    const double np_ = __builtin_fma(n.z, pol.z, __builtin_fma(n.y, pol.y, n.x * pol.x));
    const double P = __builtin_fma(-sp, sp, __builtin_fma(pol.z, pol.z, __builtin_fma(pol.y, pol.y, pol.x * pol.x)));
    tp = __builtin_fma(ns, sp, -np_);  // A_tp |m|
    const V3 e = {__builtin_fma(-ns, s.x, n.x), __builtin_fma(-ns, s.y, n.y), __builtin_fma(-ns, s.z, n.z)};
    M = __builtin_fma(e.z, e.z, __builtin_fma(e.y, e.y, e.x * e.x));
    A = P * M;
    B = tp * tp;
    bool mask = (s.x != s_.x) || (s.y != s_.y) || (s.z != s_.z);
    // Nearly parallel n and s: tp and e each carry an absolute rounding error of ~2^-53 against a magnitude of |m|, so the
    // term (tp / mm) [...] of pol', of size ~|m|, is off by ~3 * 2^-53 / |m|, and below |m| ~ 2^-26 it is noise (on a
    // tilted normal at |m| = 2^-48 a basis made there put the weight off by 4 %).  Dropping it costs at most its size:
    // there pol' = pol - (s.pol) s, ts = tp to |m|^2, and only the sum of the two squared amplitudes, P, matters -- the
    // float32 pol is unit only to 1e-7 -- split evenly.  The threshold: OT_POL_NEAR.
    // n x s == 0 exactly (a collimated beam along a face normal; s' may still differ from s by a rounding, and the
    // reference then builds its basis from the rounding noise s' x s, loses up to 2e-3 of the weight or divides 0 by 0,
    // tests/test_refraction_host.py) and s' == s bitwise keep pol and 1/2 + 1/2, the reference's contract for an
    // unchanged direction.  e does not tell: for s == n it is n (1 - n.n), a few ulps and not zero, so the exact cross
    // product is formed here, behind a wave-uniform branch that the waves of an ordinary bundle skip.  One comparison
    // more than the mask on the common path; a ballot per comparison, because each is then that comparison's own lane
    // mask (the ballot of a combined condition costs two vector instructions to form it).
    const bool near = !(M >= OT_POL_NEAR);  // NaN included
    const unsigned long long moved = __ballot(s.x != s_.x) | __ballot(s.y != s_.y) | __ballot(s.z != s_.z);
    if (__ballot(near) != 0ull || moved != __ballot(true)) {
        if (near || !mask) {
            const V3 m = cross3(n, s);
            double half = 0.5 * P;
            if (!mask || !(dot3(m, m) > 0)) {
                mask = false;
                half = 0.5;
            }
            A = 2 * half;
            B = half;
            M = 1;
            tp = 0;
        }
    }
    return mask;
}

// __compute_polarization for a surface with the same medium on both sides (N == 1, e.g. a lens whose n2 is its own n).
// There s' = s - q n with q = ns - sqrt(ns^2), which is zero or one rounding error: where it is not zero the reference
// builds its basis from ps = normalize(s' x s), a vector of rounding noise with an arbitrary direction (not even
// perpendicular to s), so A_ts^2 + A_tp^2 != |pol|^2 and the pol it stores is bent.  The result depends on every bit of
// s' x s: this is the reference's own operation order without contraction (the file's default; cross3, normalize3 and
// dot3 of ot_device.hpp are bit-exact), not the plane of incidence that refraction_polarization uses.
OT_DEV void same_medium_polarization(const V3& s, const V3& s_, const RayState& r, float& npx, float& npy, float& npz,
                                     double& A_ts2, double& A_tp2) {
    const bool mask = (s.x != s_.x) || (s.y != s_.y) || (s.z != s_.z);
    A_ts2 = 0.5;
    A_tp2 = 0.5;
    if (mask) {
        const V3 ps = normalize3(cross3(s_, s));
        const V3 pp = cross3(ps, s);
        const V3 pol = {(double)r.polx, (double)r.poly, (double)r.polz};
        const double A_ts = dot3(ps, pol), A_tp = dot3(pp, pol);
        const V3 pp_ = cross3(ps, s_);
        npx = (float)(ps.x * A_ts + pp_.x * A_tp);
        npy = (float)(ps.y * A_ts + pp_.y * A_tp);
        npz = (float)(ps.z * A_ts + pp_.z * A_tp);
        A_ts2 = A_ts * A_ts;
        A_tp2 = A_tp * A_tp;
    }
}

// Raytracer.__refraction raytracer.py:761-829 for a lane that has power and hit the surface.
// The new direction s' is computed in the reference's exact operation order (it feeds the next hit mask).
// `n` is the surface normal at the hit point, N = n1 / n2 (raytracer.py:799).  Returns true on total internal reflection.
// npx, npy, npz hold the lane's pol on entry and pol' on return.
//
// Fresnel power transmission raytracer.py:813-819 from squared amplitudes, regrouped to a single division and divided
// through by n2 (Nns = N ns is there for q anyway; n1 and n2 themselves are not needed):
//   T = n2cb/n1ca * ((A_ts*ts)^2 + (A_tp*tp)^2),  ts = 2 n1ca/(n1ca + n2cb),  tp = 2 n1ca/(n2 ns + n1 W)
//     = 4 Nns W (A_ts^2 d2^2 + A_tp^2 d1^2) / (d1 d2)^2,      d1 = Nns + W,  d2 = ns + N W
//     = 4 Nns W (A d2^2 + B (d1^2 - d2^2)) / (M (d1 d2)^2),   A = (A_ts^2 + A_tp^2) M,  B = A_tp^2 M
// (feeds only the float32 weight; see compute_polarization for the tolerance argument).  M is 1 except where
// refraction_polarization hands over its own denominator.
template <bool POL>
OT_DEV bool refract(const V3& n, RayState& r, float& wn, float& npx, float& npy, float& npz, double N) {
    V3 s = r.s;
    double ns = dot3(n, s);
    double W = ot_sqrt(1 - N * N * (1 - ns * ns));
    double Nns = N * ns;
    double q = Nns - W;
    V3 s_ = {s.x * N - n.x * q, s.y * N - n.y * q, s.z * N - n.z * q};

    double A = 1, B = 0.5, M = 1, tp, sp;  // A_ts^2 = A_tp^2 = (1/np.sqrt(2))**2
    bool bend = false;
    if (POL) {
        if (N == 1.0) {
            double A_ts2, A_tp2;
            same_medium_polarization(s, s_, r, npx, npy, npz, A_ts2, A_tp2);
            A = A_ts2 + A_tp2;
            B = A_tp2;
        } else {
            bend = refraction_polarization(n, s, s_, ns, r, A, B, M, tp, sp);
        }
    }
    // (the Fresnel terms are formed after the polarisation, not before: carried across it they cost the kernel its
    // sixth wave's registers)
    const double d1 = Nns + W, d2 = __builtin_fma(N, W, ns), den = d1 * d2;
    const double d2s = d2 * d2, den2 = den * den;
    const double rr = fast_rcp(M * den2);
    double T = 4 * (Nns * W) * (__builtin_fma(A, d2s, B * __builtin_fma(d1, d1, -d2s)) * rr);
    if (Nns == 0) T = __builtin_nan("");  // the reference divides by n1*cos(alpha)
    if (POL && bend) {
        const double k = tp * (rr * den2);  // tp / mm
        const double g = k * (1 - __builtin_fma(-q, ns, N)), h = __builtin_fma(k, W - ns, -sp);  // 1 - s.s', n.s' - n.s
        // pol is converted from its floats a second time: the empty statement hides from the compiler that it has the
        // three doubles already, which it would otherwise keep in six registers from refraction_polarization to here
        // (80 VGPRs and a spill in the bench kernel against 76 this way)
        asm("" : "+v"(npx), "+v"(npy), "+v"(npz));
        npx = (float)__builtin_fma(g, n.x, __builtin_fma(h, s.x, (double)npx));
        npy = (float)__builtin_fma(g, n.y, __builtin_fma(h, s.y, (double)npy));
        npz = (float)__builtin_fma(g, n.z, __builtin_fma(h, s.z, (double)npz));
    }
    const bool tir = !isfinite(W);
    if (tir) T = 0;
    wn = (float)((double)r.w * T);
    r.s = s_;
    return tir;
}

// Raytracer.__refraction_ideal_lens raytracer.py:720-759
template <bool POL, class SF, class EL>
OT_DEV void refract_ideal(SF& sf, EL& el, RayState& r, const V3& pn, float& npx, float& npy,
                          float& npz) {
    V3 s0 = r.s;
    double fsz = el.f / s0.z;
    V3 s = {s0.x * fsz - (pn.x - sf.px), s0.y * fsz - (pn.y - sf.py), el.f};
    s = normalize3(s);
    s.x = s.x * el.fsign;
    s.y = s.y * el.fsign;
    s.z = s.z * el.fsign;
    r.s = s;
    double A_ts, A_tp;
    compute_polarization<POL>(s0, s, r, npx, npy, npz, A_ts, A_tp);
}

// Raytracer.__outline_intersection raytracer.py:666-718 for one lane of the mask; returns true if clipped
template <class OL>
OT_DEV bool outline_clip(OL o, const V3& p, const V3& s, V3& pn, float& wn) {
    bool inside = (o[0] < pn.x) && (pn.x < o[1]) && (o[2] < pn.y) && (pn.y < o[3]) && (o[4] < pn.z) && (pn.z < o[5]);
    if (inside) return false;
    double t = __builtin_nan("");
    double T;
    T = (o[0] - p.x) / s.x; if (T > 0 && !(t <= T)) t = T;
    T = (o[1] - p.x) / s.x; if (T > 0 && !(t <= T)) t = T;
    T = (o[2] - p.y) / s.y; if (T > 0 && !(t <= T)) t = T;
    T = (o[3] - p.y) / s.y; if (T > 0 && !(t <= T)) t = T;
    T = (o[4] - p.z) / s.z; if (T > 0 && !(t <= T)) t = T;
    T = (o[5] - p.z) / s.z; if (T > 0 && !(t <= T)) t = T;
    pn = along(p, s, t);
    wn = 0.f;
    return true;
}

// Raytracer.__hurb raytracer.py:417-490 for one lane.  Returns true if the (possibly bent) direction points
// in -z (absorbed + counted; applies to every ray of the bundle, alive or not, raytracer.py:484-486).
template <bool POL, class SC, class SF>
OT_DEV bool hurb_bend(SC& sc, SF& sf, RayState& r, const V3& pn, float& wn, float& npx,
                      float& npy, float& npz, bool hwnh, double za, double zb) {
    double a_, b_;
    V3 b;
    bool inside;
    hurb_props(sf, pn.x, pn.y, a_, b_, b, inside);
    bool bend = hwnh && inside;
    V3 a = {-b.y, b.x, b.z};
    V3 s = r.s;
    double sa_ = dot3(s, a), sb_ = dot3(s, b);
    double cos_psi_a = ot_sqrt(1 - sa_ * sa_);
    double cos_psi_b = ot_sqrt(1 - sb_ * sb_);
    float wlm = r.wl * (float)1e-9;  // float32 product in the reference (wl_list is float32)
    double k = ot_div(2 * M_PI * r.n_cur, (double)wlm);
    double tan_sig_b = ot_div(sc.hurb_factor, 2 * b_ * cos_psi_b * 1e-3 * k);
    double tan_sig_a = ot_div(sc.hurb_factor, 2 * a_ * cos_psi_a * 1e-3 * k);
    double tan_tha = fabs(tan_sig_a) * za;
    double tan_thb = fabs(tan_sig_b) * zb;
    V3 sa = normalize3(cross3(b, s));
    V3 sb = cross3(s, sa);
    V3 sab = {s.x + sa.x * tan_tha + sb.x * tan_thb, s.y + sa.y * tan_tha + sb.y * tan_thb,
              s.z + sa.z * tan_tha + sb.z * tan_thb};
    V3 s0 = s;
    if (bend) {
        s = normalize3(sab);
        r.s = s;
    }
    bool neg = s.z < 0;
    if (neg) wn = 0.f;
    if (bend) {
        double A_ts, A_tp;
        compute_polarization<POL>(s0, s, r, npx, npy, npz, A_ts, A_tp);
    }
    return neg;
}

// Stores with a wave-uniform 64-bit base in SGPRs and a 32-bit per-lane byte offset: `global_store ... v_off, v_data,
// s[base]`.  Written as inline assembly because the compiler otherwise keeps one 64-bit VGPR address per stored plane
// and advances each of them every section (9 v_lshl_add_u64 per section: 3.5 % of the loop's vector instructions).
// The base is copied to a scratch SGPR pair inside the statement: a base the register allocator reloads from a spill
// slot comes out of v_readlane_b32, and a vector-memory instruction that reads an SGPR written by the vector ALU less
// than five wait states earlier uses the OLD value (gfx9 hazard).  The compiler pads that hazard for its own
// instructions but cannot see into an asm statement; a scalar move in between is interlocked by the hardware on both
// sides.  (Found as stray final directions in 1 of ~3 runs of the kernel variants that spill SGPRs.)
#ifndef OT_STORE_HINT
// Cache-policy bits of the section stores.  Every section is written once and never read by this kernel: as non-temporal
// stores they stream past the caches instead of being allocated there (A/B on one box, tools/ab_bench.py,
// profiles/r2/store_hints.txt: kernel 1.671 -> 1.622 ms with " nt"; " sc0 sc1" alone 1.667; " sc0 sc1 nt" 1.619, shipped).
#define OT_STORE_HINT " sc0 sc1 nt"
#endif
// The statements clobber "memory": they write it, and without the clobber the compiler may move its own loads and stores
// of the same planes across them (the kernel variant that loads section 0 from the planes it then overwrites).
#ifndef OT_STORE_CLOBBER
#define OT_STORE_CLOBBER : "memory"
#endif
OT_DEV void store_f64(const void* base, uint32_t off, double v) {
    const void* b;
    asm volatile("s_mov_b64 %0, %3\n\tglobal_store_dwordx2 %1, %2, %0" OT_STORE_HINT : "=&s"(b) : "v"(off), "v"(v), "s"(base) OT_STORE_CLOBBER);
}
OT_DEV void store_f32(const void* base, uint32_t off, float v) {
    const void* b;
    asm volatile("s_mov_b64 %0, %3\n\tglobal_store_dword %1, %2, %0" OT_STORE_HINT : "=&s"(b) : "v"(off), "v"(v), "s"(base) OT_STORE_CLOBBER);
}

// One section of one ray.  The plane base addresses `array + N * (section + k * nt)` are wave-uniform; the lane contributes
// the byte offsets of its ray in an f64 plane (`o8` = 8 * index) and in an f32 plane (`o4`), formed once per ray.  The
// offsets are 32 bits wide: a launch covers at most 2^28 rays (the host entry points split longer bundles and advance the
// base pointers).  The bases are 64-bit scalar arithmetic (a plane offset passes 2^32 bytes at 10 M rays; N is the padded
// plane stride), formed ON DEMAND inside the scalar branch that guards the stores they serve: the step loop carries its
// section counter and nothing else for them.  A launch that defers planes (ot_scene_set_deferred_planes: the headline
// trace writes p and w of two sections out of seventeen, neither n nor pol) then pays nothing for the sections it skips.
// Until round 10 the loop carried eight running bases and N (18 scalar registers, an add pair per base and step, advanced
// whether the section was stored or not): 46 scalar instructions per wave cheaper than the products when every section was
// stored (round 3), and dead weight since most launches store next to nothing.  Launches that still store everything are
// inside their own run-to-run range either way (profiles/r10/store_all.txt).
// Layout, measured on the bench scene, same box (profiles/r2/store_variants.txt): this form 1.676 ms, per-plane 64-bit
// VGPR addresses 1.700 ms, a wave-tiled layout ([tile of 64 rays][section][component][lane] inside each array) 1.682 ms --
// so the reference's planar Fortran layout stays and host views need no re-ordering.  Without the section stores the same
// kernel ran 1.238 ms at 2.39 GHz; with them the chip held 1.97 GHz: compute and stores do overlap, but together they ran
// into the package power limit.
// (on_demand: left to itself the compiler turns the products back into running bases -- it hoists the eight plane bases out
// of the step loop and advances two running offsets, 24 scalar registers and two add pairs per step whether the section is
// stored or not.  Behind the empty statement the section is a number it knows nothing about, so the address arithmetic
// stays inside the branch it is written in.)
OT_DEV uint32_t on_demand(int sec) {
    asm("" : "+s"(sec));
    return (uint32_t)sec;  // (a section or a section count: not negative, and 64 x 32 bits is the cheaper product)
}

// the polarisation planes of one section alone (ot_rays_fill_pol's kernel stores nothing else)
OT_DEV void store_pol(const ot_rays& R, uint32_t o4, int sec, float px, float py, float pz) {
    const uint64_t N = (uint64_t)R.N, first = N * on_demand(sec), plane = N * on_demand(R.nt);  // N * (sec + k * nt)
    store_f32(R.pol + first, o4, px);
    store_f32(R.pol + (first + plane), o4, py);
    store_f32(R.pol + (first + 2 * plane), o4, pz);
}
template <bool POL>
OT_DEV void store_section(const ot_rays& R, uint32_t o8, uint32_t o4, int sec, bool pw, const V3& p, float w, double n,
                          float px, float py, float pz) {
    // Position and weight (28 B per section): nothing between a generating trace and an image reads them before section
    // nt - 2, and such a trace can be repeated.  With OT_DEFER_SECTIONS the launcher hands in the range of sections whose
    // planes this launch writes -- [nt - 2, nt) for the trace, [0, nt - 2) for ot_rays_fill_sections -- and `pw` says
    // whether this section lies in it: section and range are wave-uniform, a scalar branch.
    if (pw) {
        const uint64_t N = (uint64_t)R.N, first = N * on_demand(sec), plane = N * on_demand(R.nt);
        store_f64(R.p + first, o8, p.x);
        store_f64(R.p + (first + plane), o8, p.y);
        store_f64(R.p + (first + 2 * plane), o8, p.z);
        store_f32(R.w + first, o4, w);
    }
    // The index plane is a function of (scene, section, wavelength) alone: with the scene's index store switched off
    // (ot_scene_set_index_store) the launcher hands in a null base, the plane stays unwritten -- 8 of 52 B per section
    // with polarisation -- and ot_rays_fill_index writes it when somebody reads it.  The base is a kernel argument: a
    // scalar branch, the same for every wave of the launch.
    if (R.n) store_f64(R.n + (uint64_t)R.N * on_demand(sec), o8, n);
    // The polarisation planes (12 of 40 B per section) are read when somebody inspects single rays, and a trace that
    // generates its rays on the device can be repeated: with OT_DEFER_POL (ot_scene_set_deferred_planes) the launcher hands
    // in a null base as well and ot_rays_fill_pol writes the planes later.  The polarisation itself is still computed: the
    // weights depend on it.
    if (POL && R.pol) store_pol(R, o4, sec, px, py, pz);
}

// The head of a step's hot record by value: kind, form, the step's indices and the ten doubles of the closed-form hit, read
// at the top of the step as one group of wide scalar loads behind one wait instead of field by field where a block uses
// them (one round trip to the scalar cache per block).  The rest of the record -- the conic constant, the ring mask, the
// normal, the ideal lens -- stays where it is and is read where it is used (HotHead: references into the record).
// The last two doubles are pinned at the top of the step (trace_ray): unpinned they sink into the conic block with a wait
// of their own.  Measured 1.1257 -> 1.1073 ms on the bench kernel, which has the scalar registers for it since the plane
// bases are formed on demand (profiles/r10/ab_arms.txt; round 8 had to leave it out for two spilled SGPRs).
struct HotHeadValues {
    int32_t kind, form, surf, n_next, filter, hurb, hurb_slot;
    double px, py, pz, r_eps2, z_max, z_lo, z_hi, k1, inv_rho, two_inv_rho;
};
template <class REC>
struct HotHead : HotHeadValues {
    decltype((((REC*)nullptr)->k)) k;
    decltype((((REC*)nullptr)->ri_eps2)) ri_eps2;
    decltype((((REC*)nullptr)->nrho)) nrho;
    decltype((((REC*)nullptr)->rho2)) rho2;
    decltype((((REC*)nullptr)->krho2)) krho2;
    decltype((((REC*)nullptr)->f)) f;
    decltype((((REC*)nullptr)->fsign)) fsign;
};
template <class REC>
OT_DEV HotHeadValues hot_head_values(REC& h) {
    return {h.kind, h.form, h.surf, h.n_next, h.filter, h.hurb, h.hurb_slot, h.px, h.py, h.pz, h.r_eps2, h.z_max, h.z_lo,
            h.z_hi, h.k1, h.inv_rho, h.two_inv_rho};
}
template <class REC>
OT_DEV HotHead<REC> hot_head(const HotHeadValues& v, REC& h) {
    return {v, h.k, h.ri_eps2, h.nrho, h.rho2, h.krho2, h.f, h.fsign};
}

// sub_trace raytracer.py:297-397 for one ray whose section 0 state is in `r`.
// The element list is flattened on the host into one STEP per tracing surface (lens front, lens back, ideal
// lens, filter, aperture), so the loop body contains a single copy of the hit search, the refraction and the
// outline clip: ~3x less code than walking elements (instruction cache) and lower register pressure.
// SPEC selects how wavelength-dependent quantities are obtained:
//   0  formulas only (no vector-memory load in the loop)      1  formulas + tabulated media / filters (global loads)
//   2  discrete spectrum: n, n1/n2 and filter T of every step were tabulated per line on the host and staged in
//      LDS (`ltab`); the lane only carries its line index.  Saves the IEEE division n1/n2 and the dispersion
//      formula per ray-surface and covers "Function" media exactly.
// `local` = index of the ray in this launch (R's pointers start at the launch's first ray), `ray` = its index in the
// whole bundle (random-number keys, injected HURB normals).
// TAIL (render-only chunks of iterative_render, trace_tail_kernel): no section is stored; `tail` receives the start of the
// LAST section (position and weight at section nt - 2), the caller takes its end from `r` -- all that a detector behind
// the last surface needs of a ray (raytracer.py:929-985).
struct TailState {
    V3 p;
    float w;
};
// What trace_ray stores: every plane (trace_kernel) / nothing, the TAIL form above / the polarisation planes alone
// (trace_pol_kernel: the replay behind ot_rays_fill_pol -- the same arithmetic, `R` needs pol, N and nt only).
// [sec_first, sec_end): with OT_STORE_ALL, the sections whose position and weight planes are written (store_section).
#define OT_STORE_ALL 0
#define OT_STORE_NONE 1
#define OT_STORE_POL 2
template <bool POL, int SPEC, int FEAT, int STORE = OT_STORE_ALL, class SC>
OT_DEV bool trace_ray(SC& sc, const ot_rays& R, uint32_t local, uint64_t ray, RayState& r,
                      const double* __restrict__ hurb_normals, uint64_t seed, unsigned int* msgs, const double* ltab,
                      int lj, double* patch_lds, TailState* tail = nullptr, int sec_first = 0,
                      int sec_end = 0x7fffffff) {
    constexpr bool TAB = (SPEC == 1);
    constexpr bool TAIL = (STORE == OT_STORE_NONE);
    constexpr bool ALL = (STORE == OT_STORE_ALL);
    constexpr bool POL_ONLY = (STORE == OT_STORE_POL);
    constexpr bool FULL = (FEAT & 1) != 0;  // HURB -- and, at hit level 0, ideal lenses and filters
    constexpr int LEVEL = FEAT / 2;         // hit level (ot_device.hpp): closed form / + Illinois search / + spline surfaces
    // Ideal lenses and filters cost 2-4 registers: the levels with a numeric hit search carry them always (their scenes
    // then need the 40-register HURB code only if they use HURB: the asphere test scene runs at 103 instead of 128
    // registers, the spline scene at three waves instead of two); level 0 keeps them behind the bit, so that the bench
    // kernel stays at 74.
    constexpr bool IDEAL_FILTER = FULL || LEVEL >= OT_HIT_ILLINOIS;
    constexpr bool NUMERIC = LEVEL >= OT_HIT_ILLINOIS;
    constexpr bool SPLINE = LEVEL >= OT_HIT_SPLINE;
    // lj = line index of this ray (SPEC == 2): found by the kernel by comparing the generated wavelength with the <= 8
    // entries of the line table in LDS (trace_kernel; seven LDS compares per ray, measured against carrying the index out of
    // generate_ray: no difference)
    const double* lrow = ltab + OT_MAX_LINES + lj;  // row 0 of this lane's column
    const uint32_t o8 = local * 8u, o4 = local * 4u;
    // numeric surfaces: this lane's coefficient patch in LDS (ot_spline.hpp::PatchCache)
    PatchCache pcache = {patch_lds + threadIdx.x, 256, nullptr};  // (spline-level launches always carry the buffer)
    PatchCache* const pc = SPLINE ? &pcache : nullptr;
    const int nt = sc.nt;
    const auto surfaces = as_const(sc.surfaces);
    const auto hot = as_const(sc.hot);
    const auto media = as_const(sc.media);
    const auto filters = as_const(sc.filters);
    const auto pool = as_const(sc.pool);
    bool ok = true;
    r.n_cur = (SPEC == 2) ? lrow[(3 * sc.n_steps) * OT_MAX_LINES] : medium_n<TAB>(media[sc.n0], pool, r.wl);
    if (ALL) store_section<POL>(R, o8, o4, 0, sec_first <= 0 && 0 < sec_end, r.p, r.w, r.n_cur, r.polx, r.poly, r.polz);
    if (POL_ONLY) store_pol(R, o4, 0, r.polx, r.poly, r.polz);

    for (int i = 0; i < sc.n_steps; i++) {  // i = index of the section the ray starts this step in
        // The step's hot record (ot_scene.hpp::HotStep): what a block of the step reads lies side by side in it, and `form`
        // says whether the record is all the step needs or the surface record is read as well.
        // Its head is read here, as one group (HotHeadValues); the empty statement keeps the group's last two doubles in it.
        auto head = hot_head_values(hot[i]);
        asm("" : "+s"(head.inv_rho), "+s"(head.two_inv_rho));
        const auto st = hot_head(head, hot[i]);
        const int form = st.form;
        if (TAIL && i + 1 == sc.n_steps) {  // the last section starts here
            tail->p = r.p;
            tail->w = r.w;
        }
        auto& sf = surfaces[st.surf];
        const int kind = st.kind;
        V3 pn = r.p;
        float wn = r.w;
        float npx = r.polx, npy = r.poly, npz = r.polz;
        const bool hw = r.w > 0;
        V3 ph;
        bool hit = false, ill = false;
        if (SPLINE) {  // another surface, another table: the cached patch and cell belong to the previous one
            pcache.key = nullptr;
        }
        if (hw) {
            if (form != OT_HOT_OTHER)
                find_hit_hot(st, form, r.p, r.s, ph, hit);
            else
                ok &= find_hit<LEVEL>(sf, r.p, r.s, ph, hit, ill, pc);
            pn = ph;
        }
        if (NUMERIC) count_event(msgs, nt, OT_INFO_ILL_COND, i + 1, hw && ill);
        const bool hwh = hw && hit, hwnh = hw && !hit;
        bool tir = false, neg = false, clip = false;
        double n_next = r.n_cur;

        if (kind <= OT_STEP_IDEAL) {  // refracting surfaces: raytracer.py:314-370
            if (hwnh) {
                wn = 0.f;
                if (kind == OT_STEP_LENS_BACK) pn = r.p;  // absorbed at the front surface, raytracer.py:354
            }
            double Nq;
            if (SPEC == 2) {
                n_next = lrow[(3 * i + 0) * OT_MAX_LINES];
                Nq = lrow[(3 * i + 1) * OT_MAX_LINES];
            } else {
                n_next = medium_n<TAB>(media[st.n_next], pool, r.wl);
                Nq = ot_div(r.n_cur, n_next);
            }
            if (hwh) {
                if (IDEAL_FILTER && kind == OT_STEP_IDEAL) {
                    refract_ideal<POL>(st, st, r, pn, npx, npy, npz);
                } else {
                    // pn is a hit point: is_hit implies mask(pn) (surface.py:409)
                    V3 n;
                    if (form != OT_HOT_OTHER)
                        n = hot_normal(st, form, pn.x, pn.y);
                    else
                        n = surf_normal<true, LEVEL>(sf, pn.x, pn.y, pc);
                    tir = refract<POL>(n, r, wn, npx, npy, npz, Nq);
                }
            }
        } else if (IDEAL_FILTER && kind == OT_STEP_FILTER) {  // raytracer.py:379-380
            if (hwh) {
                double T = (SPEC == 2) ? lrow[(3 * i + 2) * OT_MAX_LINES] : filter_T<TAB>(filters[st.filter], pool, r.wl);
                wn = (float)((double)r.w * T);
            }
        } else {  // aperture raytracer.py:381-386
            if (hwh) wn = 0.f;
            if (FULL && st.hurb) {
                double za, zb;
                if (TAB && hurb_normals) {
                    za = (hurb_normals + (2 * (int64_t)st.hurb_slot + 0) * R.N)[ray];
                    zb = (hurb_normals + (2 * (int64_t)st.hurb_slot + 1) * R.N)[ray];
                } else {
                    philox_normal2(seed, ray, 0x48555242u, (uint32_t)st.hurb_slot, za, zb);
                }
                neg = hurb_bend<POL>(sc, sf, r, pn, wn, npx, npy, npz, hwnh, za, zb);
            }
            if (FULL) count_event(msgs, nt, OT_INFO_HURB_NEG_DIR, i + 1, neg);
        }
        // rays that missed the surface may leave the outline box on their way (raytracer.py:338, 367, 389)
        if (hwnh) clip = outline_clip(sc.outline, r.p, r.s, pn, wn);
        // the rare events of a step are counted behind one wave-wide test (a surface that every ray of the wave hits
        // and passes has none)
        if (__ballot(hwnh || tir) != 0ull) {
            if (kind <= OT_STEP_IDEAL) {
                count_event(msgs, nt, OT_INFO_ABSORB_MISSING, i + 1, hwnh);
                count_event(msgs, nt, OT_INFO_TIR, i, tir);
            }
            count_event(msgs, nt, OT_INFO_OUTLINE_INTERSECTION, i, clip);
        }

        r.p = pn;
        r.w = wn;
        r.polx = npx;
        r.poly = npy;
        r.polz = npz;
        r.n_cur = n_next;
#ifdef OT_NO_SECTION_STORES  // experiment (tools/power_clock.py): the same arithmetic, only the last section is stored
        if (i + 1 == sc.n_steps)
#endif
        {
            if (ALL)
                store_section<POL>(R, o8, o4, i + 1, sec_first <= i + 1 && i + 1 < sec_end, r.p, r.w, r.n_cur, r.polx,
                                   r.poly, r.polz);
            if (POL_ONLY) store_pol(R, o4, i + 1, r.polx, r.poly, r.polz);
        }
    }
    if (ALL) {
        const int64_t N = R.N;
        store_f64(R.s, o8, r.s.x);
        store_f64(R.s + N, o8, r.s.y);
        store_f64(R.s + 2 * N, o8, r.s.z);
    }
    return ok;
}
