// The Shrake-Rupley point test of one atom and the atom table it reads, for the kernels that must agree on it dot for dot:
// iface_points_kernel (interface.hip) counts the points, shape_dots_kernel (shape.hip) turns the same points into dots and marks a
// structure whose counts disagree with `points`.  One definition, so the two cannot drift apart.
//
// Every test is float64 without fused multiply-add, a squared distance is (dx * dx + dy * dy) + dz * dz: the counts are exact integers,
// equal to those of abx_amd.interface.interface_host.  Rounding cannot make the prefilter drop an occluder: a point lies within 1e-12
// of R_a from its centre, so an occluding atom has d <= R_a + R_b + 1e-12, six orders inside the slack.
#pragma once
#include "common.h"
#include "reduce_dev.h"

#pragma clang fp contract(off)

constexpr int CAP = 192;               // neighbour list entries per wave (worked off when fewer than 64 are free)
constexpr double SLACK = 1e-3;         // Angstrom added to R_a + R_b in the neighbour prefilter
constexpr double FOUR_PI = 12.566370614359172;

// area of the n of P sphere points of an atom whose radius with the probe is R
__device__ __forceinline__ double points_area(double R, double n, double P) { return (FOUR_PI * (R * R)) * n / P; }

// The table entry of atom14 slot k (row * 14 + slot) of a structure: the atom exists with a positive radius -> x, y, z, radius;
// tag = slot index << 1 | side.  Without the atom `at` is zero (its w too: no radius bits).
template <class Structure>
__device__ __forceinline__ bool table_entry(const Structure& s, int k, int Lab, float4& at, int& tag) {
    const int row = k / 14, sl = k - row * 14, aa = s.aatype(row);
    const float r = s.radius[aa * 14 + sl];
    const bool ok = r > 0.f && s.exists(row, sl, aa);
    at = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
        const float* x = s.xyz(row, sl);
        at = make_float4(x[0], x[1], x[2], r);
    }
    tag = (k << 1) | (row >= Lab ? 1 : 0);
    return ok;
}

// dynamic LDS of a kernel with `waves` waves that holds the table of L rows: float4 and tag per slot, a neighbour list per wave
__host__ __device__ constexpr long long table_lds_bytes(int L, int waves) { return 14ll * L * 20 + (long long)waves * CAP * 4; }

// The table of one structure in LDS.  The constructor is called by the whole workgroup (it ends with a barrier).
struct TableLds {
    float4* tab;                       // [n] x, y, z, radius
    int* tag;                          // [n] slot index << 1 | side
    int* list;                         // this wave's neighbours: table index | other side << 31
    int n;
    __device__ __forceinline__ TableLds(unsigned char* lds, int L, int threads, const float4* gtab, const int* gtag, int n_) : n(n_) {
        const int N14 = L * 14, tid = threadIdx.x;
        tab = reinterpret_cast<float4*>(lds);
        tag = reinterpret_cast<int*>(lds + 16ll * N14);
        list = reinterpret_cast<int*>(lds + 20ll * N14) + (tid >> 6) * CAP;
        for (int i = tid; i < n; i += threads) {
            tab[i] = gtab[i];
            tag[i] = gtag[i];
        }
        __syncthreads();
    }
};

// bit k of a mask: this lane's point k * 64 + lane.  alive: occluded by no own-side atom; crossed: occluded by an other-side one
struct PointMasks {
    unsigned alive, crossed;
    int contacts;                      // CONTACTS, side-A atom: this lane's other-side atoms within the cutoff (sum over the wave)
};

// The P points of table atom ia against the table, by one wave.  It scans the table 64 atoms per step - the conservative sphere-sphere
// test d < R_a + R_b + SLACK - and appends the neighbours by ballot to the wave's list.  Its lanes take the points lane, lane + 64,
// ... and walk the list: an own-side occluder ends the point (it is lost to every surface), an other-side occluder is only recorded.
// A list that fills up is worked off and reused: no bound on the neighbours.  The scan ends when no point is alive - but with
// CONTACTS a side-A atom scans on to the end of the table, adding no neighbour: the contacts still need it.
template <bool CONTACTS>
__device__ __forceinline__ PointMasks point_test(const TableLds& t, int ia, const double* __restrict__ sphere, int P, double probe, double cut2) {
    const int lane = threadIdx.x & 63, n = t.n, npass = (P + 63) >> 6;
    const float4* tab = t.tab;
    int* list = t.list;
    const float4 me = tab[ia];
    const int mside = t.tag[ia] & 1;
    const double xa = (double)me.x, ya = (double)me.y, za = (double)me.z, Ra = (double)me.w + probe;
    unsigned alive = 0, crossed = 0;
    for (int k = 0; k < npass; ++k) alive |= (k * 64 + lane < P ? 1u : 0u) << k;
    int cnt = 0, ncontact = 0;

    // the points of this atom against the cnt neighbours of the list
    auto work_off = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // the list entries of the other lanes (one wave: in order)
        __builtin_amdgcn_wave_barrier();
        for (int k = 0; k < npass; ++k) {
            bool live = (alive >> k) & 1u;
            if (__ballot(live) == 0ull) continue;
            const int p = min(k * 64 + lane, P - 1);
            const double px = xa + Ra * sphere[3 * p], py = ya + Ra * sphere[3 * p + 1], pz = za + Ra * sphere[3 * p + 2];
            bool cross = false;
            for (int j = 0; j < cnt; ++j) {
                const int e = list[j];
                const float4 o = tab[e & 0x7fffffff];
                const double dx = px - (double)o.x, dy = py - (double)o.y, dz = pz - (double)o.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const double Rb = (double)o.w + probe;
                if (live && d2 < Rb * Rb) {
                    if (e < 0) cross = true;
                    else live = false;
                }
                if (__ballot(live) == 0ull) break;
            }
            if (!live) alive &= ~(1u << k);
            if (cross) crossed |= 1u << k;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // the list is free again
    };

    bool dead = false;                                  // no point is left
    for (int base = 0; base < n; base += 64) {
        if (dead && (!CONTACTS || mside != 0)) break;
        const int j = base + lane;
        bool nb = false, other = false;
        if (j < n && j != ia) {
            const float4 o = tab[j];
            other = (t.tag[j] & 1) != mside;
            const double dx = xa - (double)o.x, dy = ya - (double)o.y, dz = za - (double)o.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const double rs = (Ra + ((double)o.w + probe)) + SLACK;
            nb = !dead && d2 < rs * rs;
            if (CONTACTS && other && mside == 0 && d2 < cut2) ++ncontact;
        }
        const unsigned long long bal = __ballot(nb);
        if (nb) list[cnt + lanes_below(bal)] = j | (other ? (int)0x80000000 : 0);
        cnt += __popcll(bal);
        if (cnt > CAP - 64) {
            work_off();
            cnt = 0;
            dead = __ballot(alive != 0u) == 0ull;
        }
    }
    if (cnt > 0) work_off();                            // (cnt is 0 once no point is alive: nothing is appended after that)
    return PointMasks{alive, crossed, ncontact};
}
