// rtg_trav.hpp — device code shared by the render kernels (rtg_kernels.hip) and the ray-query kernels
// (rtg_query.hip): the rtg-f32 vector and transcendental forms, the primitive tests (sphere_t, quad_t, tri_t)
// with the exact-t tie rule, the per-lane traversal state and stacks, and the node and leaf steps. Everything
// sits in an unnamed namespace, so each translation unit compiles its own copy under its own flags.
#pragma once
#include <cstdint>

#include "rtg_internal.hpp"
#include "rtg_numerics.hpp"

namespace rtg {
namespace {

constexpr float kTMin = 0.001f;  // interval(0.001, infinity), camera.hpp:192
// Conservative culling. Box tests only prune: a child is skipped when
// its entry distance is past fmaf(tbest, kCullRel, kCullAbs) or its exit before kCullTMin, a margin at
// least the oracle's (oracle/cpu_ref.c node_hit32: tbest (1 + 1e-6) + 1e-6, floor 0.0009), while the
// primitive tests keep the exact tbest and tmin. With the boxes padded on the host for the slab test's
// rounding (rtg_api.cpp pad_down), a box holding the closest hit is never culled by fp32 error.
constexpr float kCullTMin = 0.0009f;
constexpr float kCullRel = 1.0f + 0x1p-19f;
constexpr float kCullAbs = 0x1p-19f;
__device__ __forceinline__ float cull_bound(float tbest) { return fmaf(tbest, kCullRel, kCullAbs); }
// Kernels that test quads compare a child's entry distance with min(exit, tbest) * kCullWiden instead: the
// slab test's relative error (3 2^-24 of t per plane) and quad_t's (2 2^-24) are then taken in t, so the boxes
// need padding only for the errors that do not grow with the distance (rtg_api.cpp culling_box), and the
// factor is the cull bound's relative margin as well (its absolute 2^-19 is covered by the pads there). One
// v_pk_mul_f32 per child pair replaces cull_bound. Sphere-only kernels keep cull_bound and the plain exit
// (their boxes carry the distance terms).
constexpr float kCullWiden = 1.0f + 0x1p-19f;
constexpr float kPi = 3.14159265358979323846f;
constexpr int kMaxTexNesting = 16;

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 mul(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 scl(float t, V3 a) { return v3(t * a.x, t * a.y, t * a.z); }
__device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
// Fused multiply-adds of the rtg-f32 spec (round 2): dot products, cross products,
// `b + t a` and the other forms below are single-rounding fmaf chains in exactly this order, here
// and in oracle/cpu_ref.c (fmaf is correctly rounded on both sides, so the bits still agree).
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return v3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
__device__ __forceinline__ V3 madd(float t, V3 a, V3 b) {  // b + t a
  return v3(fmaf(t, a.x, b.x), fmaf(t, a.y, b.y), fmaf(t, a.z, b.z));
}
__device__ __forceinline__ V3 vfma(V3 a, V3 b, V3 c) {  // a * b + c per component
  return v3(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z));
}
// div_rn / sqrt_rn: rtg_numerics.hpp (shared with the numerics check, tests/native)
__device__ __forceinline__ V3 unit(V3 a) {  // unit_vector: v / v.length() == (1/len) * v
  const float len = sqrt_rn(dot(a, a));
  return scl(div_rn(1.0f, len), a);
}
__device__ __forceinline__ V3 xyz(float4 f) { return v3(f.x, f.y, f.z); }
__device__ __forceinline__ int ibits(float f) { return __float_as_int(f); }

// ---------------------------------------------------------------------------------------
// Counter RNG: a 64-bit LCG (PCG's multiplier and increment) seeded per
// (pixel, sample) by a splitmix64 finaliser; a draw is the top 24 bits of the advanced state.
// Replaces the global glibc rand() stream (rtweekend.hpp:23-39, hazard H1). Round 1 drew PCG32
// XSH-RR outputs; the top bits of the 64-bit state are as good for 24-bit uniforms (G5 tests)
// at 7 VALU per draw instead of ~14.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}
// One draw's 24 bits as an exact float integer in [0, 2^24): uniform() = draw24() * 2^-24. Callers that
// scale U by a power of two or add a constant fold the scaling into one exact product (and the constant
// into an fmaf, whose one rounding is the spec's rounding of the sum): bit-identical, fewer VALU ops.
__device__ __forceinline__ float draw24(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  // bits 63..40, converted by an explicit v_cvt_f32_u32: the compiler widens a plain
  // (float)(uint32_t)(s >> 40) back into a 64-bit integer-to-float expansion (+6 VALU per draw)
  const uint32_t top = static_cast<uint32_t>(s >> 32) >> 8;
  float f;
  asm("v_cvt_f32_u32 %0, %1" : "=v"(f) : "v"(top));
  return f;
}
__device__ __forceinline__ float uniform(uint64_t& s) {  // random_double(), [0,1), 24 bits
  return draw24(s) * 5.9604644775390625e-8f;
}

// sin and cos of 2*pi*u, u in [0,1): quadrant reduction and Taylor polynomials on [-pi/4, pi/4),
// plain fp32 multiply / fmaf only, so oracle/cpu_ref.c (sincos_turn) reproduces every bit. Takes
// t = 4u (for a draw: draw24 * 2^-22, the spec's 4 * (draw24 * 2^-24) exactly)
__device__ __forceinline__ void sincos_turn4(float t, float& sn, float& cs) {
  const float q = floorf(t);
  const float x = (t - q - 0.5f) * 1.57079637f;
  const float x2 = x * x;
  // Horner steps as fmaf (rtg-f32 round 2)
  const float ps = fmaf(x2, fmaf(x2, fmaf(x2, 2.75573188e-6f, -1.98412701e-4f), 8.33333377e-3f), -1.66666672e-1f);
  const float sx = fmaf(x * x2, ps, x);
  const float pc = fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, -2.75573188e-7f, 2.48015876e-5f), -1.38888892e-3f),
                                 4.16666679e-2f), -0.5f);
  const float cx = fmaf(x2, pc, 1.0f);
  const float a = (sx + cx) * 0.707106769f;  // sin(pi/4 + x)
  const float b = (cx - sx) * 0.707106769f;  // cos(pi/4 + x)
  const int qi = static_cast<int>(q);
  const float c0 = (qi & 1) ? a : b, s0 = (qi & 1) ? b : a;
  cs = (qi == 1 || qi == 2) ? -c0 : c0;
  sn = (qi >= 2) ? -s0 : s0;
}

// The textures' transcendentals in the rtg-f32 spec (round 3). libm's sinf / acosf / atan2f (ocml
// here, glibc in the oracle) differ in the last ulp, which left ~26 % of config 3's pixels off the
// oracle by ~1e-6. These are fixed sequences of fp32 operations (fmaf, correctly rounded division and
// square root, rint), restated in oracle/cpu_ref.c, so the GPU and the oracle agree to the bit.
// sin: Cody-Waite reduction by pi/2 in three fmaf steps, then Cephes' sinf / cosf polynomials on
// [-pi/4, pi/4] (about 1 ulp for |x| < 8192; the noise texture's argument is scale * z + 10 * turb).
__device__ __forceinline__ float sin_spec(float x) {
  const float k = rintf(x * 0x1.45f306p-1f);  // nearest multiple of pi/2
  float r = fmaf(-k, 0x1.921fb6p+0f, x);
  r = fmaf(-k, -0x1.777a5cp-25f, r);
  r = fmaf(-k, -0x1.ee59dap-50f, r);
  const float z = r * r;
  const float sr = fmaf(fmaf(fmaf(-0x1.9943f2p-13f, z, 0x1.11073cp-7f), z, -0x1.555546p-3f) * z, r, r);
  const float cr = fmaf(fmaf(fmaf(0x1.99eb9cp-16f, z, -0x1.6c0c34p-10f), z, 0x1.55554ap-5f), z * z,
                        fmaf(-0.5f, z, 1.0f));
  // the quadrant k mod 4 in float (exact for every integer-valued k; NaN / inf fall to 0), so no
  // float -> int conversion sees an out-of-range value here or in the oracle. The spec's
  // accuracy claim is |x| < 8192 (three-step reduction); larger arguments stay bit-identical between
  // kernel and oracle but drift from libm's sin.
  const float m = k - 4.0f * floorf(0.25f * k);
  const int q = (m >= 0.0f && m < 4.0f) ? static_cast<int>(m) : 0;
  const float v = (q & 1) ? cr : sr;
  return (q & 2) ? -v : v;
}
// atan2: the ratio of the smaller to the larger magnitude, above tan(pi/8) shifted by pi/4, Cephes'
// atanf polynomial, then the octant; the sign follows y (atan2(+-0, x >= +0) = +-0, x < 0: +-pi)
__device__ __forceinline__ float atan2_spec(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  const float a = mn > 0x1p-100f ? div_rn(mn, mx) : 0.0f;  // div_rn's exact range (and atan ~ 0 below)
  const bool big = a > 0x1.a8279ap-2f;  // tan(pi/8)
  const float t = big ? div_rn(a - 1.0f, a + 1.0f) : a;
  const float z = t * t;
  float r = fmaf(fmaf(fmaf(fmaf(0x1.49e1a2p-4f, z, -0x1.1c370ap-3f), z, 0x1.9924bep-3f), z, -0x1.555454p-2f) * z,
                 t, t);
  if (big) r = r + 0x1.921fb6p-1f;      // + pi/4
  if (ay > ax) r = 0x1.921fb6p+0f - r;  // pi/2 - r
  if (x < 0.0f) r = 0x1.921fb6p+1f - r; // pi - r
  return copysignf(r, y);
}
// acos v = atan2(sqrt(1 - v^2), v), v in [-1, 1]
__device__ __forceinline__ float acos_spec(float v) {
  return atan2_spec(sqrtf(fmaxf(0.0f, fmaf(-v, v, 1.0f))), v);
}

// random_unit_vector (vec3.hpp:172-184) by direct sampling (DESIGN.md rtg-f32): z = 1 - 2U, then
// the azimuth from a second U. The reference's rejection loop would make every wave wait for its
// unluckiest lane (~5 tries for 30 lanes at acceptance pi/6); this costs two draws, always.
__device__ __forceinline__ V3 random_unit_vector(uint64_t& s) {
  const float z = fmaf(-0x1p-23f, draw24(s), 1.0f);  // 1 - 2U: 2U = draw24 * 2^-23 exactly
  const float r = sqrt_rn(fmaxf(0.0f, fmaf(-z, z, 1.0f)));
  float sn, cs;
  sincos_turn4(draw24(s) * 0x1p-22f, sn, cs);
  return v3(r * cs, r * sn, z);
}

// ---------------------------------------------------------------------------------------
// Geometry
// sphere::hit (sphere.hpp:47-93) with the fp32-robust root form of DESIGN.md: c = |oc|^2 - r^2
// is formed in f64 for spheres of radius >= kSphereF64Radius (a ground sphere, where fp32
// cancellation would put self-hits above tmin), in fp32 below it, where the discriminant is
// taken from the centre-to-line distance; the near root is c/q. Returns the root or -1.
// `origin`: the ray starts on this sphere (its previous segment hit it): only the far root of a
// ray entering the sphere counts (DESIGN.md §4 "origin rule"; fp32 puts the origin ~ulp(|p|) off
// the surface, and a grazing ray's own root could pass tmin and trap a reflection inside).
// (kSphereF64Radius: rtg_internal.hpp, shared with the host's occluder constants)
// a = d.d and inv_a = 1/a (correctly rounded) are per ray (Trav): the far root is q * inv_a and
// only the near root c / q is a division.
// The roots of a sphere test from its c, discriminant and half-b (the part of sphere_t after the two chains)
template <bool INCL>
__device__ __forceinline__ float sphere_roots(float c, float disc, float hb, float a, float inv_a, float tmin,
                                              float tmax, bool origin) {
  if (disc < 0.0f) return -1.0f;
  const float sq = sqrtf(disc);
  const float q = -(hb + copysignf(sq, hb));
  // |q| < 2^-100 (a ray tangent at its own origin, q would otherwise have no lower bound) counts as a
  // miss in the rtg-f32 spec (oracle/cpu_ref.c the same): div_rn is exact for every divisor left, and
  // the guard is the compare the q == 0 test already made (div_rn_wide, which scaled tiny
  // divisors instead, cost earth_perlin 4-6 % in register allocation, profiles/r03_c/ab_div_*)
  if (fabsf(q) < 0x1p-100f || a == 0.0f) return -1.0f;
  const float t0 = q * inv_a;
  const float t1 = div_rn(c, q);
  const float lo = fminf(t0, t1);
  const float hi = fmaxf(t0, t1);
  // roots inside (tmin, tmax), interval::surrounds (sphere.hpp:70); INCL: (tmin, tmax], so that the leaf test
  // sees a root equal to the closest hit and applies the exact-t tie rule (DESIGN.md §4 "tie rule")
  if (origin) return (hb < 0.0f && tmin < hi && (INCL ? hi <= tmax : hi < tmax)) ? hi : -1.0f;
  if (tmin < lo && (INCL ? lo <= tmax : lo < tmax)) return lo;
  if (tmin < hi && (INCL ? hi <= tmax : hi < tmax)) return hi;
  return -1.0f;
}

template <bool INCL = false>
__device__ __forceinline__ float sphere_t(float4 s0, float4 s1, V3 o, V3 d, float a, float inv_a, float time,
                                          float tmin, float tmax, bool origin) {
  const V3 C = madd(time, xyz(s1), xyz(s0));
  const V3 oc = sub(o, C);
  const float hb = dot(oc, d);
  float c, disc;
  if (fabsf(s0.w) < kSphereF64Radius) {
    c = fmaf(-s0.w, s0.w, dot(oc, oc));
    // disc = a (r^2 - |f|^2), f = oc - (h/a) d the centre-to-line offset: no h^2 - a c
    // cancellation, so a grazing ray far from a small sphere is classified to ~r^2 2^-22, not
    // ~h^2 2^-24 (a false hit outside the sphere's box, which box culling precision then decides)
    const float s = hb * inv_a;
    const V3 f = madd(-s, d, oc);
    disc = a * fmaf(s0.w, s0.w, -dot(f, f));
  } else {
    const double ox = static_cast<double>(o.x) - static_cast<double>(C.x);
    const double oy = static_cast<double>(o.y) - static_cast<double>(C.y);
    const double oz = static_cast<double>(o.z) - static_cast<double>(C.z);
    const double r = static_cast<double>(s0.w);
    // r * r of a float r is exact in f64, so the fma's one rounding is the subtraction's
    c = static_cast<float>(fma(-r, r, ox * ox + oy * oy + oz * oz));
    disc = fmaf(hb, hb, -(a * c));
  }
  return sphere_roots<INCL>(c, disc, hb, a, inv_a, tmin, tmax, origin);
}

// Scene classes a kernel is compiled for (PRIMS): bits 0-1 the primitives its leaf test and shading
// handle — any (the scene's ref_mode decides at run time), spheres only, quads only, triangles only — and
// bit 2 set when no material is metal or dielectric. Bit 3 (kPrimsTriMix, with kPrimsAny): the scene holds
// triangles beside other primitives, or triangles that the triangle-only class does not serve (cache-read
// schedules, binary trees, 32-bit stacks): the mixed leaf test and shading carry the triangle branch. The
// kernels without the bit are compiled exactly as before triangles existed. The small-scene / dual-launch LDS kernels are built per class so
// a scene's kernel carries no code for what the scene lacks (default_kernel).
constexpr int kPrimsAny = 0, kPrimsSpheres = 1, kPrimsQuads = 2, kPrimsTris = 3, kPrimsKind = 3, kPrimsDiffuse = 4, kPrimsTriMix = 8;

// quad::hit (quad.hpp:44-114); plane distance D - n.O formed in f64.
// `rank`: the quad's list index (its record's v.w, DESIGN.md §4 "tie rule"), set with a hit. `brank`: the
// closest hit's rank (-1: a sphere or none); a root equal to tmax is a miss unless this quad comes later
// in the list than that hit (exact-t tie rule; compared on the hit path only). brank = -2: no tie check
// (the cache-read schedules settle ties after the call)
__device__ __forceinline__ float quad_t(const float4* q, V3 o, V3 d, float tmin, float tmax, int32_t brank,
                                        int32_t& rank) {
  const float4 q0 = q[0], q4 = q[4];
  const V3 n = xyz(q4);
  const float denom = dot(n, d);
  if (fabsf(denom) < 1e-8f) return -1.0f;
  // products of two floats are exact in f64, so the fma chain rounds exactly where mul + add would
  const double dn = fma(static_cast<double>(n.z), static_cast<double>(o.z),
                        fma(static_cast<double>(n.y), static_cast<double>(o.y),
                            static_cast<double>(n.x) * static_cast<double>(o.x)));
  const float num = static_cast<float>(static_cast<double>(q0.w) - dn);
  const float t = div_rn(num, denom);
  if (!(tmin <= t && t <= tmax)) return -1.0f;
  const V3 p = madd(t, d, o);
  const V3 hp = sub(p, xyz(q0));
  const float4 q2 = q[2];
  const V3 u = xyz(q[1]), v = xyz(q2), w = xyz(q[3]);
  const float alpha = dot(w, cross(hp, v));
  const float beta = dot(w, cross(u, hp));
  if (!(0.0f <= alpha && alpha <= 1.0f) || !(0.0f <= beta && beta <= 1.0f)) return -1.0f;
  rank = ibits(q2.w);
  if (t == tmax && rank <= brank) return -1.0f;
  return t;
}

// Exact-t ties (rtg-f32 spec, DESIGN.md §4 "tie rule"). The reference tests the world's objects in
// list order (hittable_list.hpp:40-64) against a shrinking interval: quad::hit accepts t ==
// closest_so_far (interval::contains, quad.hpp:62, interval.hpp:29), sphere::hit does not
// (interval::surrounds, sphere.hpp:70, interval.hpp:32). So among the primitives at the smallest t it
// keeps the last quad of the list if there is one, else the first sphere, whatever order they are tested
// in. The kernels test in BVH order: quad_t returns roots up to tmax, and a quad root equal to the closest
// hit replaces it only if that hit is a sphere or an earlier quad of the list (S.tie_rank: each slot's list
// index, read only on a tie; the check is one compare and a wave-uniform branch); the leaf tests take sphere
// roots up to tmax too (sphere_t<true>), and a sphere root equal to the closest hit replaces it only if that
// hit is a sphere later in the list, again with the ranks read only on a tie (tie_ranks_late). The sphere
// half (round 5) decides 14 pixels of the 10 M of configs 2 and 5 at full spp at no net cost (earlier forms
// that carried ranks through the loop cost 2-8 %: tools/experiments/sphere_tie_rule.patch).
__device__ __forceinline__ uint64_t ballot_tie(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// S.tie_rank for the sphere tie rule, read from the kernel arguments at the (rare) tie itself: every kernel
// that runs leaf_step (render_kernel, render_kernel_lds) takes its DevScene as the first argument. A volatile
// load there keeps the pointer out of the SGPRs live across the trip loop; with S.tie_rank instead the
// compiler held it from the kernel's start and spilled other scalars to VGPR lanes (config 2 +0.7 %,
// config 3 +4.5 %, config 5 +1.2 %, frames identical)
__device__ __forceinline__ const int32_t* tie_ranks_late() {
  const volatile DevScene* ks = (const volatile DevScene*)(__builtin_amdgcn_kernarg_segment_ptr());
  return ks->tie_rank;
}
// The counting (COUNT) kernels check that assumption at every tie: a kernel whose first argument
// is not its DevScene reads another pointer there, reported as a corrupt render (rtg_render: RTG_E_INVALID);
// they then use S.tie_rank itself
template <bool COUNT>
__device__ __forceinline__ const int32_t* tie_ranks_at_tie(const DevScene& S, bool& corrupt) {
  const int32_t* r = tie_ranks_late();
  if (COUNT && r != S.tie_rank) {
    corrupt = true;
    return S.tie_rank;
  }
  return r;
}
// DevJob::tile_order read from the kernel arguments where a batch is handed out, as tie_ranks_late reads the
// tie ranks: J.tile_order itself was held in SGPRs from the kernel's start and pushed other scalars into VGPR
// lanes (config 2 +1 % with the order off). Every kernel that runs render_stream takes (DevScene, DevCamera,
// DevJob) by value, so DevJob sits at the offset below in the kernel-argument segment (arguments in order, each
// at its own alignment); the COUNT kernels compare the two pointers and report a mismatch as corrupt.
constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
constexpr size_t kDevJobKernarg =
    align_up(align_up(sizeof(DevScene), alignof(DevCamera)) + sizeof(DevCamera), alignof(DevJob));
template <bool COUNT>
__device__ __forceinline__ const int32_t* tile_order_late(const DevJob& J, bool& corrupt) {
  const char* ka = (const char*)(__builtin_amdgcn_kernarg_segment_ptr());
  const uint64_t v = reinterpret_cast<uint64_t>(
      *reinterpret_cast<const int32_t* const volatile*>(ka + kDevJobKernarg + offsetof(DevJob, tile_order)));
  // the load is a vector load: its (uniform) value back into SGPRs, so the null test is a scalar branch
  const int32_t* r = reinterpret_cast<const int32_t*>(
      (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32)))) << 32) |
      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v & 0xffffffffu))));
  if (COUNT && r != J.tile_order) {
    corrupt = true;
    return J.tile_order;
  }
  return r;
}
// A wave-uniform kernel argument read where it is used: a volatile load through the constant address space is
// a scalar load (s_load_dword..x16) issued at that point, so the value holds no SGPR from the kernel's start
// across the trip loop (the compiler otherwise loads every argument once, first thing, and spills what does
// not fit to VGPR lanes). Offsets come from offsetof / sizeof of the parameter structs only: every kernel that
// runs render_stream takes (DevScene, DevCamera, DevJob) by value, each at its own alignment.
typedef __attribute__((address_space(4))) const char karg_bytes;
template <class T>
__device__ __forceinline__ T karg(size_t off) {
  karg_bytes* ka = (karg_bytes*)(__builtin_amdgcn_kernarg_segment_ptr());
  return *reinterpret_cast<const volatile __attribute__((address_space(4))) T*>(ka + off);
}
typedef int karg_i4 __attribute__((ext_vector_type(4)));
typedef int karg_i8 __attribute__((ext_vector_type(8)));
typedef float karg_f4 __attribute__((ext_vector_type(4)));
typedef float karg_f8 __attribute__((ext_vector_type(8)));
typedef double karg_d4 __attribute__((ext_vector_type(4)));
constexpr size_t kDevSceneKernarg = 0;
constexpr size_t kDevCameraKernarg = align_up(sizeof(DevScene), alignof(DevCamera));
static_assert(kDevJobKernarg == align_up(kDevCameraKernarg + sizeof(DevCamera), alignof(DevJob)),
              "kernel arguments: DevScene, DevCamera, DevJob in that order");
static_assert(offsetof(DevScene, occ) % 8 == 0 && offsetof(DevOccluder, cd) == 0 && offsetof(DevOccluder, r2) == 24 &&
                  offsetof(DevOccluder, c) == 32 && offsetof(DevOccluder, r) == 44 &&
                  offsetof(DevOccluder, index) == 48 && offsetof(DevOccluder, mode) == 52 &&
                  offsetof(DevOccluder, mat) == 56,
              "DevOccluder is read as {double4 cd + r2}, {float4 c + r}, {int4 index, mode, mat}");

// The occluder (DevScene::occluder: the scene-spanning sphere kept out of the BVH) against one segment, as
// sphere_t(record, o, d, ..., kTMin, tbest, origin == occluder) computes it. With DevOccluder::mode != 0 the record
// loads, the centre at `time`, the widened centre, r * r and the radius branch are the host's constants (the same
// operations on the same operands: DESIGN.md §4 "occluder constants"); every operation that involves the ray is
// the one sphere_t runs, in its order. mode 0 runs sphere_t itself. Returns the root or -1; `ref`, `mat`: the occluder's sphere index and material.
template <bool COUNT>
__device__ __forceinline__ float occluder_t(const DevScene& S, V3 o, V3 d, float a, float inv_a, float time,
                                            float tmax, int32_t origin, int32_t& ref, int32_t& mat, bool& corrupt) {
  constexpr size_t kOcc = kDevSceneKernarg + offsetof(DevScene, occ);
  const karg_i4 k = karg<karg_i4>(kOcc + offsetof(DevOccluder, index));  // index, mode, mat
  if (COUNT && (k.x != S.occ.index || k.y != S.occ.mode)) corrupt = true;  // (the first argument is not the DevScene)
  if (k.x < 0) return -1.0f;
  ref = k.x;
  if (k.y == 0) {
    const float4* sp4 = S.spheres + static_cast<int64_t>(k.x) * S.sphere_f4;
    const float4 s1 = sp4[1];
    mat = ibits(s1.w);
    return sphere_t(sp4[0], s1, o, d, a, inv_a, time, kTMin, tmax, k.x == origin);
  }
  mat = k.z;
  const karg_f4 cr = karg<karg_f4>(kOcc + offsetof(DevOccluder, c));  // centre, radius
  const V3 oc = sub(o, v3(cr.x, cr.y, cr.z));
  const float hb = dot(oc, d);
  float c, disc;
  if (k.y == 1) {
    c = fmaf(-cr.w, cr.w, dot(oc, oc));
    const float s = hb * inv_a;
    const V3 f = madd(-s, d, oc);
    disc = a * fmaf(cr.w, cr.w, -dot(f, f));
  } else {
    const karg_d4 cd = karg<karg_d4>(kOcc + offsetof(DevOccluder, cd));  // widened centre, r * r
    const double ox = static_cast<double>(o.x) - cd.x;
    const double oy = static_cast<double>(o.y) - cd.y;
    const double oz = static_cast<double>(o.z) - cd.z;
    // sphere_t's fma(-r, r, sum): r * r is exact in f64, so its one rounding is this subtraction's
    c = static_cast<float>((ox * ox + oy * oy + oz * oz) - cd.w);
    disc = fmaf(hb, hb, -(a * c));
  }
  return sphere_roots<false>(c, disc, hb, a, inv_a, kTMin, tmax, k.x == origin);
}

// Cache-read schedules (Trav::mat holds the hit's material): the closest hit's rank is re-read from the
// list ranks (a triangle's from its cold record), only on a tie (wave-uniform branch). Quads and triangles alike.
template <bool TRIS = false>
__device__ __forceinline__ bool quad_wins_tie(const DevScene& S, int32_t qrank, int32_t best) {
  if (TRIS && (best & kTriRefBit)) return qrank > S.tri_meta[best & kRefSlotMask].y;
  if (!(best & kQuadRefBit)) return true;
  return qrank > S.tie_rank[S.num_spheres + (best & ~kQuadRefBit)];
}

// Triangle (RTG_PRIM_TRIANGLE; rtg-f32 spec, DESIGN.md §4 "triangles"): the plane-form record T = {n.xyz, D},
// {A.xyz, a0}, {B.xyz, b0}. t exactly as quad_t forms it (so a triangle coplanar with a quad gives the
// bit-identical root), accepted in [tmin, tmax]; then the two edge-plane evaluations at p = o + t d,
// alpha = A.p + a0 and beta = B.p + b0, each an fma chain in the x, y, z order of dot() that starts from the
// constant. Inside: alpha >= 0, beta >= 0, alpha + beta <= 1. Returns the root or -1; ties (root == tmax)
// are settled by the caller.
__device__ __forceinline__ float tri_edge(float4 e, V3 p) { return fmaf(e.z, p.z, fmaf(e.y, p.y, fmaf(e.x, p.x, e.w))); }
__device__ __forceinline__ float tri_t(const float4* T, V3 o, V3 d, float tmin, float tmax) {
  const float4 t0 = T[0];
  const V3 n = xyz(t0);
  const float denom = dot(n, d);
  if (fabsf(denom) < 1e-8f) return -1.0f;
  const double dn = fma(static_cast<double>(n.z), static_cast<double>(o.z),
                        fma(static_cast<double>(n.y), static_cast<double>(o.y),
                            static_cast<double>(n.x) * static_cast<double>(o.x)));
  const float num = static_cast<float>(static_cast<double>(t0.w) - dn);
  const float t = div_rn(num, denom);
  if (!(tmin <= t && t <= tmax)) return -1.0f;
  const V3 p = madd(t, d, o);
  const float alpha = tri_edge(T[1], p);
  const float beta = tri_edge(T[2], p);
  if (!(alpha >= 0.0f && beta >= 0.0f && alpha + beta <= 1.0f)) return -1.0f;
  return t;
}
template <bool COUNT>
struct Counts {
  uint32_t box = 0, prim = 0;
  uint32_t spill = 0;  // stack pushes into the global spill area (counters[26])
};

// Per-lane traversal state of the child-pair BVH (replaces hittable_list::hit -> bvh_node::hit
// -> aabb::hit, hittable_list.hpp:40-64, bvh_node.hpp:80-94, aabb.hpp:61-112). Ordered
// traversal: the nearer child first, the farther one pushed on the lane's LDS stack.
struct Trav {
  float ix, iy, iz;  // 1/d (approximate: culling only)
  float a, inv_a;    // d.d and its correctly rounded reciprocal (sphere_t)
  float ox, oy, oz;  // -o/d, for the fused slab test
  int32_t sx, sy, sz;  // 4-wide nodes: byte offset (0 or 48) of each axis' near-plane row
  float tbest;    // closest hit so far (the shrinking interval.max of the reference)
  int32_t best;   // primitive ref of the closest hit, -1 = none
  int32_t todo;   // inner node (>= 0: index, or byte offset in 4-wide trees) or leaf code (< 0)
  int32_t sp;     // stack depth
  int32_t origin; // primitive ref the ray starts on (-1: camera ray), DESIGN.md §4 "origin rule"
  int32_t mat;    // material of the closest hit: the cache-read schedules' shading then fetches the
                  // material beside the primitive instead of after it (one memory round trip less);
                  // in the LDS schedule instead the closest hit's tie rank (a quad's list index, -1
                  // for a sphere or none: the exact-t tie rule)
};

// todo of a finished traversal. "Traversal active" is this integer compare, not a bool of its own:
// a bool carried around the trip loop becomes a lane mask that every ballot copies into a VGPR and
// compares back (2 VALU per ballot); a compare of todo feeds s_bcnt1 / the exec mask directly.
constexpr int32_t kTravDone = INT32_MAX;
__device__ __forceinline__ bool trav_active(const Trav& t) { return t.todo != kTravDone; }
__device__ __forceinline__ bool at_inner(const Trav& t) {  // 0 <= todo < kTravDone
  return static_cast<uint32_t>(t.todo) < static_cast<uint32_t>(kTravDone);
}

template <int WIDE = 4>
__device__ __forceinline__ void trav_begin(Trav& t, const DevScene& S, V3 o, V3 d, int32_t origin) {
  t.ix = __builtin_amdgcn_rcpf(d.x);
  t.iy = __builtin_amdgcn_rcpf(d.y);
  t.iz = __builtin_amdgcn_rcpf(d.z);
  if constexpr (WIDE == 2) {
    // The child-pair slab test (node_step) takes min / max of a slab's two plane distances. A direction
    // component of exactly 0 (or a denormal) gives 1/d = inf, and plane * inf - o * inf is NaN for every plane
    // on the origin's side of 0 but -inf for a plane below 0 (a wall at 0 padded outward): max(-inf, NaN) = -inf
    // then culls a box the ray runs inside of, from the root down, and the ray leaves the scene. Finite
    // reciprocals (|1/d| <= 2^100) keep both distances finite with the right signs; the test only culls, so
    // nothing else changes. The 4-wide test picks near and far planes by the sign of 1/d and ignores the NaN.
    t.ix = __builtin_amdgcn_fmed3f(t.ix, -0x1p100f, 0x1p100f);
    t.iy = __builtin_amdgcn_fmed3f(t.iy, -0x1p100f, 0x1p100f);
    t.iz = __builtin_amdgcn_fmed3f(t.iz, -0x1p100f, 0x1p100f);
  }
  // byte offset of the far-plane rows (hi.x after lo.x, ...) in 4-wide nodes
  constexpr int32_t kHalf = 48;
  t.sx = (static_cast<uint32_t>(ibits(t.ix)) >> 31) * kHalf;
  t.sy = (static_cast<uint32_t>(ibits(t.iy)) >> 31) * kHalf;
  t.sz = (static_cast<uint32_t>(ibits(t.iz)) >> 31) * kHalf;
  t.a = dot(d, d);
  t.inv_a = div_rn(1.0f, t.a);
  t.ox = -o.x * t.ix;
  t.oy = -o.y * t.iy;
  t.oz = -o.z * t.iz;
  t.tbest = __builtin_inff();
  t.best = -1;
  t.mat = -1;  // no hit: tie rank -1 (LDS schedule; the cache-read schedules overwrite it on a hit)
  t.todo = S.num_nodes > 0 ? S.root_code : kTravDone;
  t.sp = 0;
  t.origin = origin;
}

// Per-lane traversal stacks, laid out [depth][lane] (bank-conflict-free ds_read/write_b32).
// LdsStack: all N entries in LDS. SpillStack: the first N entries in LDS, deeper ones (deep BVHs
// only, e.g. the 1M-sphere scene's 36-entry bound) in a global per-wave area of the same layout,
// so the LDS part stays small enough for full occupancy and no tree is too deep.
template <int N>
struct LdsStack {
  int32_t* lds;
  __device__ __forceinline__ bool spills(int32_t) const { return false; }
  __device__ __forceinline__ int32_t capacity() const { return N; }
  __device__ __forceinline__ void store(int32_t sp, int32_t v) const { lds[sp * 64] = v; }
  __device__ __forceinline__ int32_t load(int32_t sp) const { return lds[sp * 64]; }
};
// LdsStack16: 16-bit entries for the LDS schedule of 4-wide trees whose codes fit an int16: the node
// array sits at LDS address 0, so inner-node codes (absolute LDS byte addresses) stay below 32768
// for trees of <= 292 nodes, and leaf codes ~((first << 3) | (count - 1)) need first < 4096 (the host
// checks both, the kernel re-checks the node range): half the LDS of 32-bit entries, which is what
// lets a second persistent launch share the CU with book-1 (DESIGN.md §3 "occupancy").
template <int N>
struct LdsStack16 {
  int16_t* lds;
  __device__ __forceinline__ bool spills(int32_t) const { return false; }
  __device__ __forceinline__ int32_t capacity() const { return N; }
  __device__ __forceinline__ void store(int32_t sp, int32_t v) const { lds[sp * 64] = static_cast<int16_t>(v); }
  __device__ __forceinline__ int32_t load(int32_t sp) const { return lds[sp * 64]; }
};
template <int N>
struct SpillStack {
  int32_t* lds;
  int32_t* spill;  // this lane's global area, entries n.. at spill[(sp - n) * 64]
  int32_t n;       // entries kept in LDS (<= N; J.lds_stack, lowered only by tests)
  int32_t cap;     // n + spill depth
  __device__ __forceinline__ bool spills(int32_t sp) const { return sp >= n; }
  __device__ __forceinline__ int32_t capacity() const { return cap; }
  __device__ __forceinline__ void store(int32_t sp, int32_t v) const {
    if (__builtin_expect(sp < n, 1))
      lds[sp * 64] = v;
    else
      spill[(sp - n) * 64] = v;
  }
  __device__ __forceinline__ int32_t load(int32_t sp) const {
    int32_t v;
    if (__builtin_expect(sp < n, 1))
      v = lds[sp * 64];
    else
      v = spill[(sp - n) * 64];
    return v;
  }
};

template <class Stk>
__device__ __forceinline__ void trav_pop(Trav& t, const Stk& stk) {
  if (t.sp == 0) {
    t.todo = kTravDone;
    return;
  }
  --t.sp;
  t.todo = stk.load(t.sp);
}

// Visit one inner node (t.todo >= 0): test both child boxes, continue with the nearer hit child
// and push the farther one, or pop when neither is hit.
template <class Stk, bool COUNT>
__device__ __forceinline__ void node_step(Trav& t, const DevScene& S, const Stk& stk, Counts<COUNT>& cnt,
                                          bool& overflow, bool& corrupt, float tfloor = kCullTMin) {
  if (t.todo >= S.num_nodes) {  // corrupt child code: report, never read out of bounds
    corrupt = true;
    t.todo = kTravDone;
    return;
  }
  const float4* n = S.nodes + static_cast<int64_t>(t.todo) * 4;
  const float4 a = n[0], b = n[1], c = n[2];
  const int4 ch = *reinterpret_cast<const int4*>(n + 3);
  if (COUNT) cnt.box += 2;
  const V3 inv = v3(t.ix, t.iy, t.iz), oi = v3(t.ox, t.oy, t.oz);
  // left box lo=(a.x,a.y,a.z) hi=(a.w,b.x,b.y); right lo=(b.z,b.w,c.x) hi=(c.y,c.z,c.w)
  const float l0x = fmaf(a.x, inv.x, oi.x), l1x = fmaf(a.w, inv.x, oi.x);
  const float l0y = fmaf(a.y, inv.y, oi.y), l1y = fmaf(b.x, inv.y, oi.y);
  const float l0z = fmaf(a.z, inv.z, oi.z), l1z = fmaf(b.y, inv.z, oi.z);
  const float r0x = fmaf(b.z, inv.x, oi.x), r1x = fmaf(c.y, inv.x, oi.x);
  const float r0y = fmaf(b.w, inv.y, oi.y), r1y = fmaf(c.z, inv.y, oi.y);
  const float r0z = fmaf(c.x, inv.z, oi.z), r1z = fmaf(c.w, inv.z, oi.z);
  const float tc = cull_bound(t.tbest);
  const float ln = fmaxf(fmaxf(fminf(l0x, l1x), fminf(l0y, l1y)), fmaxf(fminf(l0z, l1z), tfloor));
  const float lf = fminf(fminf(fminf(fmaxf(l0x, l1x), fmaxf(l0y, l1y)), fmaxf(l0z, l1z)) * kCullWiden, tc);
  const float rn = fmaxf(fmaxf(fminf(r0x, r1x), fminf(r0y, r1y)), fmaxf(fminf(r0z, r1z), tfloor));
  const float rf = fminf(fminf(fminf(fmaxf(r0x, r1x), fmaxf(r0y, r1y)), fmaxf(r0z, r1z)) * kCullWiden, tc);
  // An empty slot (right child only; the host guarantees the left one is never empty) has an
  // inverted box, which the symmetric min/max slab form would report as all of space: test
  // the child code explicitly.
  const bool hl = ln <= lf;
  const bool hr = rn <= rf && ch.y != kEmptyChild;
  if (hl && hr) {
    const bool lfirst = ln <= rn;
    if (COUNT) cnt.spill += stk.spills(t.sp) ? 1u : 0u;
    if (t.sp < stk.capacity()) {
      stk.store(t.sp, lfirst ? ch.y : ch.x);
      ++t.sp;
    } else {
      overflow = true;
    }
    t.todo = lfirst ? ch.x : ch.y;
  } else if (hl || hr) {
    t.todo = hl ? ch.x : ch.y;
  } else {
    trav_pop(t, stk);
  }
}

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float nf4 __attribute__((ext_vector_type(4)));
// LDS loads from 32-bit LDS byte addresses (no generic-pointer base arithmetic)
__device__ __forceinline__ nf4 lds_ld4(uint32_t a) {
  return *reinterpret_cast<__attribute__((address_space(3))) const nf4*>(static_cast<uintptr_t>(a));
}
__device__ __forceinline__ int32_t lds_ld1(uint32_t a) {
  return *reinterpret_cast<__attribute__((address_space(3))) const int32_t*>(static_cast<uintptr_t>(a));
}
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// Entry distance of one child (tn) or a miss: the slab test with the near/far planes already
// chosen by the ray's direction signs, so no min/max between a slab's two planes is needed.
// tc: the cull bound of the closest hit so far (cull_bound)
__device__ __forceinline__ uint32_t child_key(float tnx, float tny, float tnz, float tfx, float tfy, float tfz,
                                              float tc, uint32_t slot, float tfloor = kCullTMin) {
  const float tn = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), tfloor);
  const float tf = fminf(fminf(fminf(tfx, tfy), tfz), tc);
  // tn >= kCullTMin > 0, so its bits order like the float; the low 4 bits carry the slot (x4)
  return tn <= tf ? ((static_cast<uint32_t>(ibits(tn)) & ~15u) | slot) : ~0u;
}
// the same with the bound already formed (quad kernels: min(exit, tbest) * kCullWiden)
__device__ __forceinline__ uint32_t child_key_exit(float tnx, float tny, float tnz, float tf, uint32_t slot,
                                                   float tfloor = kCullTMin) {
  const float tn = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), tfloor);
  return tn <= tf ? ((static_cast<uint32_t>(ibits(tn)) & ~15u) | slot) : ~0u;
}

__device__ __forceinline__ void psort(uint32_t& ka, int32_t& ca, uint32_t& kb, int32_t& cb) {
  const bool sw = kb < ka;
  const uint32_t k = sw ? kb : ka;
  const int32_t c = sw ? cb : ca;
  kb = sw ? ka : kb;
  cb = sw ? ca : cb;
  ka = k;
  ca = c;
}

__device__ __forceinline__ void usort(uint32_t& a, uint32_t& b) {
  const uint32_t lo = min(a, b);
  b = max(a, b);
  a = lo;
}

// Visit one 4-wide node (SoA rows lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, code; 16 B each). Per ray
// the near plane of each axis is fixed by the sign of 1/d (Trav::sx/sy/sz pick the row), so each
// child costs 6 fma (packed two children per v_pk_fma_f32) + max3/max + min3/min. The four hit
// children are sorted as integer keys (entry distance with the slot in the low bits) by a
// 5-comparator min/max network; the nearest becomes the next node, the others are pushed
// far-to-near. Empty slots hold the inverted box (+inf, -inf): whatever the signs, at least one
// axis has a finite 1/d, for which the near plane gives tn = +inf and the far one tf = -inf, so an
// empty slot can never be entered (rays with all three components zero do not exist).
// Node geometry of a schedule: where node rows are read from.
enum Geom : int {
  kGeomLds = 0,      // whole scene in LDS; inner codes are absolute LDS addresses, codes read after the sort
  kGeomGlobal = 1,   // scene through the caches; codes travel with their keys through the sort network
  kGeomTreelet = 2,  // nodes below S.treelet_bytes from their LDS copy, the rest through the caches
};

// WIDEN (kernels that test quads): exit distances widened by kCullWiden (DESIGN.md §4 "conservative culling").
template <class Stk, bool COUNT, int GEOM, bool WIDEN = true>
__device__ __forceinline__ void node_step4(Trav& t, const DevScene& S, const Stk& stk, Counts<COUNT>& cnt,
                                           bool& overflow, bool& corrupt, float tfloor = kCullTMin) {
  constexpr bool PAIRS = GEOM != kGeomLds;
  // 4-wide inner-node codes are byte offsets into the node array (node index * 112)
  // corrupt codes: checked wherever a bad code could fault (nodes through the vector-memory path)
  // and in the COUNT diagnostics; an LDS read outside the allocation cannot fault, and the host
  // validated the tree it copied there, so the hot LDS schedule skips the compare-and-branch
  if ((GEOM != kGeomLds || COUNT) && t.todo >= S.node_limit) {
    corrupt = true;
    t.todo = kTravDone;
    return;
  }
  // the probe of the hot treelet counts every visit of a node held in HBM (rtg_api.cpp tune_treelet)
  if (COUNT && GEOM != kGeomLds && S.node_visits) atomicAdd(S.node_visits + t.todo / 112, 1u);
  const char* nb = reinterpret_cast<const char*>(S.nodes) + t.todo;
  const int32_t sx = t.sx, sy = t.sy, sz = t.sz;
  const uint32_t na = static_cast<uint32_t>(t.todo);  // LDS scenes: the node's LDS address
  nf4 nx, ny, nz, fx, fy, fz;
  int4 cc;
  if constexpr (GEOM == kGeomLds) {
    nx = lds_ld4(na + sx), ny = lds_ld4(na + 16 + sy), nz = lds_ld4(na + 32 + sz);
    fx = lds_ld4(na + 48 - sx), fy = lds_ld4(na + 64 - sy), fz = lds_ld4(na + 80 - sz);
  } else {
    if (GEOM == kGeomTreelet && t.todo < S.treelet_bytes) {  // the top of the tree: a ds_read
      const uint32_t la = S.treelet_lds + na;
      nx = lds_ld4(la + sx), ny = lds_ld4(la + 16 + sy), nz = lds_ld4(la + 32 + sz);
      fx = lds_ld4(la + 48 - sx), fy = lds_ld4(la + 64 - sy), fz = lds_ld4(la + 80 - sz);
      const nf4 c4 = lds_ld4(la + 96);
      cc = *reinterpret_cast<const int4*>(&c4);
    } else {
      auto row = [&](int32_t off) -> nf4 { return *reinterpret_cast<const nf4*>(nb + off); };
      nx = row(sx), ny = row(16 + sy), nz = row(32 + sz);
      fx = row(48 - sx), fy = row(64 - sy), fz = row(80 - sz);
      cc = *reinterpret_cast<const int4*>(nb + 96);
    }
  }
  if (COUNT) cnt.box += 4;
  const f2 ix = {t.ix, t.ix}, iy = {t.iy, t.iy}, iz = {t.iz, t.iz};
  const f2 ox = {t.ox, t.ox}, oy = {t.oy, t.oy}, oz = {t.oz, t.oz};
  const f2 nx01 = pk_fma(f2{nx.x, nx.y}, ix, ox), nx23 = pk_fma(f2{nx.z, nx.w}, ix, ox);
  const f2 ny01 = pk_fma(f2{ny.x, ny.y}, iy, oy), ny23 = pk_fma(f2{ny.z, ny.w}, iy, oy);
  const f2 nz01 = pk_fma(f2{nz.x, nz.y}, iz, oz), nz23 = pk_fma(f2{nz.z, nz.w}, iz, oz);
  const f2 fx01 = pk_fma(f2{fx.x, fx.y}, ix, ox), fx23 = pk_fma(f2{fx.z, fx.w}, ix, ox);
  const f2 fy01 = pk_fma(f2{fy.x, fy.y}, iy, oy), fy23 = pk_fma(f2{fy.z, fy.w}, iy, oy);
  const f2 fz01 = pk_fma(f2{fz.x, fz.y}, iz, oz), fz23 = pk_fma(f2{fz.z, fz.w}, iz, oz);
  uint32_t k0, k1, k2, k3;
  if constexpr (WIDEN) {  // min(exit, tbest) * kCullWiden: one v_pk_mul_f32 per child pair, no cull_bound
    const float tb = t.tbest;
    const f2 tf01 = f2{fminf(fminf(fminf(fx01.x, fy01.x), fz01.x), tb), fminf(fminf(fminf(fx01.y, fy01.y), fz01.y), tb)} *
                    f2{kCullWiden, kCullWiden};
    const f2 tf23 = f2{fminf(fminf(fminf(fx23.x, fy23.x), fz23.x), tb), fminf(fminf(fminf(fx23.y, fy23.y), fz23.y), tb)} *
                    f2{kCullWiden, kCullWiden};
    k0 = child_key_exit(nx01.x, ny01.x, nz01.x, tf01.x, 0, tfloor);
    k1 = child_key_exit(nx01.y, ny01.y, nz01.y, tf01.y, 4, tfloor);
    k2 = child_key_exit(nx23.x, ny23.x, nz23.x, tf23.x, 8, tfloor);
    k3 = child_key_exit(nx23.y, ny23.y, nz23.y, tf23.y, 12, tfloor);
  } else {
    const float tc = cull_bound(t.tbest);
    k0 = child_key(nx01.x, ny01.x, nz01.x, fx01.x, fy01.x, fz01.x, tc, 0, tfloor);
    k1 = child_key(nx01.y, ny01.y, nz01.y, fx01.y, fy01.y, fz01.y, tc, 4, tfloor);
    k2 = child_key(nx23.x, ny23.x, nz23.x, fx23.x, fy23.x, fz23.x, tc, 8, tfloor);
    k3 = child_key(nx23.y, ny23.y, nz23.y, fx23.y, fy23.y, fz23.y, tc, 12, tfloor);
  }
  if constexpr (PAIRS) {
    // scene in global memory: the codes travel with their keys through the network, so no second
    // memory round trip sits between the sort and the next node load (-3.6 % on config 5; with
    // the scene in LDS the extra selects cost more than the LDS latency they save)
    int32_t c0 = cc.x, c1 = cc.y, c2 = cc.z, c3 = cc.w;
    psort(k0, c0, k1, c1);
    psort(k2, c2, k3, c3);
    psort(k0, c0, k2, c2);
    psort(k1, c1, k3, c3);
    psort(k1, c1, k2, c2);
    if (k0 == ~0u) {
      trav_pop(t, stk);
      return;
    }
    const int npush = (k1 != ~0u) + (k2 != ~0u) + (k3 != ~0u);
    if (COUNT)
      for (int j = 0; j < npush; ++j) cnt.spill += stk.spills(t.sp + j) ? 1u : 0u;
    if (t.sp + npush > stk.capacity()) {
      overflow = true;
    } else {
      if (k3 != ~0u) stk.store(t.sp++, c3);
      if (k2 != ~0u) stk.store(t.sp++, c2);
      if (k1 != ~0u) stk.store(t.sp++, c1);
    }
    t.todo = c0;
  } else {
    usort(k0, k1);
    usort(k2, k3);
    usort(k0, k2);
    usort(k1, k3);
    usort(k1, k2);
    if (k0 == ~0u) {
      trav_pop(t, stk);
      return;
    }
    // node addresses are 16-byte aligned (112-byte nodes from an aligned base), so the code of
    // slot (k & 12) / 4 is at (node | (k & 12)) + 96: one v_and_or per code
    auto code_of = [&](uint32_t k) { return lds_ld1((na | (k & 12u)) + 96u); };
    // the host sizes every stack from the tree's structural bound (sum of siblings along a path,
    // Bvh4::max_pushes), so pushes cannot overflow; the check runs in the COUNT diagnostics only
    const int npush = (k1 != ~0u) + (k2 != ~0u) + (k3 != ~0u);
    if (COUNT)
      for (int j = 0; j < npush; ++j) cnt.spill += stk.spills(t.sp + j) ? 1u : 0u;
    if (COUNT && t.sp + npush > stk.capacity()) {
      overflow = true;
    } else {
      if (k3 != ~0u) stk.store(t.sp++, code_of(k3));
      if (k2 != ~0u) stk.store(t.sp++, code_of(k2));
      if (k1 != ~0u) stk.store(t.sp++, code_of(k1));
    }
    t.todo = code_of(k0);
  }
}

// Test the primitives of a leaf (t.todo < 0). ONE: only the first, and the lane stays at the rest of the leaf
// (first + 1, count - 1) for its next leaf trip, or pops after the last: one primitive per lane per trip
// keeps the leaf trip's lanes in step (a loop over each lane's own count runs as long as the wave's largest
// leaf): config 2 -0.5 %, config 5 -0.4 %, Cornell +0.3 %, frames identical. The tile-ring kernels of the
// cache-read schedules loop over the leaf and pop (config 5 with the ring: one per trip +1.4 %; DESIGN.md §8
// round 5). Either way a lane tests its primitives in the same order, so ties resolve the same way. CHECK:
// validate the leaf code (off in the LDS schedule outside the COUNT diagnostics, as for node codes).
// QRY (the ray-query kernels, rtg_query.hip; 0: a render): the interval's lower end is the ray's own `tmin`
// and t.tbest starts at the ray's tmax with no hit behind it (t.best < 0), so a root equal to it is no tie: a
// sphere's is outside (tmin, tmax), a quad's or triangle's inside [tmin, tmax]. kQueryAny: the lane's traversal
// ends at its first accepted root (an occlusion query).
constexpr int kQueryClosest = 1, kQueryAny = 2;
template <class Stk, bool COUNT, bool CHECK = true, bool MAT = false, int WIDE = 4, int GEOM = kGeomLds,
          int PRIMS = kPrimsAny, bool ONE = true, int QRY = 0>
__device__ __forceinline__ void leaf_step(Trav& t, const DevScene& S, V3 o, V3 d, float time,
                                          const Stk& stk, Counts<COUNT>& cnt, bool& corrupt, float tmin = kTMin) {
  auto pop = [&]() { trav_pop(t, stk); };
  // a root equal to the closest hit so far (QRY: only when there is one)
  auto tie = [&](float th) { return th == t.tbest && (QRY == 0 || t.best >= 0); };
  // the leaf's primitives are done (ANY: the query's answer is in)
  auto next = [&](int32_t first, int32_t count) {
    if (QRY == kQueryAny && t.best >= 0)
      t.todo = kTravDone;
    else if (ONE && count > 1)
      t.todo = ~(((first + 1) << 3) | (count - 2));
    else
      pop();
  };
  constexpr bool kTriMix = (PRIMS & kPrimsTriMix) != 0;  // the mixed path tests triangles too
  const int32_t code = ~t.todo;
  const int32_t first = code >> 3;
  const int32_t count = (code & 7) + 1;
  if ((CHECK || COUNT) && static_cast<int64_t>(first) + count > S.num_refs) {
    corrupt = true;
    t.todo = kTravDone;
    return;
  }
  if constexpr ((PRIMS & kPrimsKind) == kPrimsTris) {
    // triangle-only scene, records in reference order (ref = slot, no kind bit): three 16-B rows per test,
    // nothing else; the cold record {material, rank} is read on a hit (MAT) or on an exact-t tie only
    for (int k = 0; k < (ONE ? 1 : count); ++k) {
      const int32_t slot = first + k;
      if (COUNT) cnt.prim += 1;
      // planar: a ray leaving a triangle never hits it again
      const float th = slot == t.origin ? -1.0f : tri_t(S.tris + static_cast<int64_t>(slot) * 3, o, d, tmin, t.tbest);
      bool take = th > 0.0f;
      // exact-t tie (rare; a wave-uniform branch): the triangle later in the list wins (interval::contains)
      if (ballot_tie(tie(th)) != 0 && tie(th)) take = S.tri_meta[slot].y > S.tri_meta[t.best].y;
      if (take) {
        t.tbest = th;
        t.best = slot;
        t.mat = MAT ? S.tri_meta[slot].x : -1;
      }
    }
    next(first, count);
    return;
  }
  if ((PRIMS & kPrimsKind) == kPrimsSpheres || ((PRIMS & kPrimsKind) == kPrimsAny && S.ref_mode == 1)) {  // sphere-only scene, primitives stored in reference order
    for (int k = 0; k < (ONE ? 1 : count); ++k) {
      const float4* sp4 = S.spheres + static_cast<int64_t>(first + k) * S.sphere_f4;
      if (COUNT) cnt.prim += 1;
      const float th = sphere_t<true>(sp4[0], sp4[1], o, d, t.a, t.inv_a, time, tmin, t.tbest, first + k == t.origin);
      // exact-t tie (rare; a wave-uniform branch): the sphere earlier in the list wins, as the reference's list
      // walk keeps the first sphere at a t (interval::surrounds); the ranks are read only then (tie_ranks_late)
      bool take = th > 0.0f && th < t.tbest;
      if (ballot_tie(tie(th)) != 0 && tie(th)) {
        const int32_t* rk = tie_ranks_at_tie<COUNT>(S, corrupt);
        take = rk[first + k] < rk[t.best];
      }
      if (take) {
        t.tbest = th;
        t.best = first + k;
        t.mat = MAT ? ibits(sp4[1].w) : -1;
      }
    }
    next(first, count);
    return;
  }
  for (int k = 0; k < (ONE ? 1 : count); ++k) {
    const int32_t ref = S.ref_mode == 0 ? S.refs[first + k] : ((first + k) | (kTriMix && S.ref_mode == 3 ? kTriRefBit : kQuadRefBit));
    float th;
    if (COUNT) cnt.prim += 1;
    int32_t m = 0, qrank = -1;
    bool take;
    if ((PRIMS & kPrimsKind) == kPrimsQuads || (ref & kQuadRefBit)) {  // planar: a ray leaving a quad never hits it again
      const float4* q = S.quads + static_cast<int64_t>(ref & ~kQuadRefBit) * 5;
      // exact-t tie rule: a quad root equal to the closest hit replaces it only if that
      // is a sphere or an earlier quad of the list. LDS schedule: t.mat holds the closest hit's rank and
      // quad_t rejects a losing tie on its hit path; cache-read schedules (t.mat = material): the rank
      // is re-read, only on a tie
      th = ref == t.origin ? -1.0f : quad_t(q, o, d, tmin, t.tbest, MAT ? -2 : t.mat, qrank);
      if (MAT && th > 0.0f) m = ibits(q[1].w);
      take = th > 0.0f;
      if constexpr (MAT) {
        if (ballot_tie(tie(th)) != 0 && tie(th)) take = quad_wins_tie<kTriMix>(S, qrank, t.best);
      }
    } else if (kTriMix && (ref & kTriRefBit)) {  // planar, as a quad
      const int32_t slot = ref & kRefSlotMask;
      th = ref == t.origin ? -1.0f : tri_t(S.tris + static_cast<int64_t>(slot) * 3, o, d, tmin, t.tbest);
      take = th > 0.0f;
      // the cold record on a hit: the material (cache-read schedules) or the list rank, which a later quad or
      // triangle at the same t is compared with (LDS schedule: t.mat, as for a quad)
      if (th > 0.0f) {
        const int2 cold = S.tri_meta[slot];
        m = cold.x;
        qrank = cold.y;
      }
      if (ballot_tie(tie(th)) != 0 && tie(th)) take = MAT ? quad_wins_tie<true>(S, qrank, t.best) : qrank > t.mat;
    } else {
      const float4* sp4 = S.spheres + static_cast<int64_t>(ref) * S.sphere_f4;
      th = sphere_t<true>(sp4[0], sp4[1], o, d, t.a, t.inv_a, time, tmin, t.tbest, ref == t.origin);
      if (MAT) m = ibits(sp4[1].w);
      take = th > 0.0f && th < t.tbest;
      // exact-t tie: a sphere replaces only an equal-t sphere later in the list (never a quad or triangle)
      if (ballot_tie(tie(th)) != 0 && tie(th)) {
        const int32_t* rk = tie_ranks_at_tie<COUNT>(S, corrupt);
        take = !(t.best & (kQuadRefBit | (kTriMix ? kTriRefBit : 0))) && rk[ref] < rk[t.best];
      }
    }
    if (take) {  // th > tmin >= 0.001 on a hit
      t.tbest = th;
      t.best = ref;
      t.mat = MAT ? m : qrank;
    }
  }
  next(first, count);
}

}  // namespace
}  // namespace rtg
