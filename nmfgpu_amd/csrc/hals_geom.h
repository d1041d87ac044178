// hals_geom.h -- the lane mapping of the HALS sweep kernels, shared by k_sweep_hals (kernels_hals.hip: one sweep per launch) and k_sweeps_hals
// (kernels_hals_multi.hip: several sweeps per launch), so that both cut a panel into the same workgroups and write the same number of partial
// sums of squares (panel_sweep_hals_parts).  docs/HALS.md describes the mapping.
#pragma once

#include <stddef.h>

namespace nmfamd {

template <typename T, int RP>
struct HalsShape;
// L: lanes per column (a power of two, E = RP / L entries per lane: 8 ... 16); C: columns per lane group
template <int RP> struct HalsShape<float, RP> { static constexpr int L = RP <= 64 ? 4 : RP <= 128 ? 8 : RP <= 256 ? 16 : 32; static constexpr int C = RP <= 128 ? 1 : 2; };
template <int RP> struct HalsShape<double, RP> { static constexpr int L = RP <= 64 ? 4 : RP <= 128 ? 8 : RP <= 256 ? 16 : 32; static constexpr int C = RP <= 128 ? 1 : 2; };

constexpr int HALS_THREADS = 256;

template <typename T, int RP>
struct HalsGeom {
	static constexpr int L = HalsShape<T, RP>::L, C = HalsShape<T, RP>::C, E = RP / L;
	static constexpr int GROUPS = HALS_THREADS / L, COLS = GROUPS * C;
	// rows of G per LDS chunk: all of G where it fits 64 KiB
	static constexpr int KC = (int)(65536 / (RP * sizeof(T))) < RP ? (int)(65536 / (RP * sizeof(T))) : RP;
	static_assert(RP % L == 0 && E <= 16, "entries per lane");
	static_assert(COLS <= KC && 128 % COLS == 0, "the sum-of-squares staging reuses the G chunk; workgroups tile 128-column panels");
};

} // namespace nmfamd
