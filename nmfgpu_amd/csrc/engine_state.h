// engine_state.h -- which derived buffers of an Engine still describe its current W, H and V (internal header; plain C++17, no device code).  The iteration
// families (materialize_w, iterate_*, tri_*, h_step_impl, ...) own their state machines and write the flags directly; whatever replaces a factor or V from
// OUTSIDE an iteration goes through one of the named transitions below -- a new derived buffer is remembered here, once.
#pragma once

#include <initializer_list>

namespace nmfamd {

struct PanelState {
	// rank-64 MU fast path: W is kept unnormalised with a pending column scale (kernels_mu64.hip)
	bool fused_ready = false, w_pending = false;
	bool h_product_ahead = false, f64_product_ahead = false;   // begin_next_iteration() has enqueued the W^T V launch of the next iterate_mu64 / iterate_fused64 (it reads W and V)
	bool f32w_pending = false, f64_pending = false;   // fused fp32 (padded ranks >= 128) / fp64 iteration: Wt_ unnormalised, sumsq_part_ holds its sums of squares (fp32: Wx3_ its split image)
	bool kl_scale_pending = false;     // KL iteration: Wt_ holds the unnormalised result of the last KL W update (materialize_w folds kl_scale_ in)
	bool kl_sw_ready = false;          // sW_ holds the column sums of the current W (left by its last KL update; a W set from outside needs the pass over the panel)
	bool gram_w_ready = false;         // generic rank-64 fp32 path: G_ holds W^T W of the current (normalised) W
	bool wx3_valid = false, hx3_valid = false;   // Wx3_ / Hx3_ hold the split image of the current Wt_ / H_
	bool wtb_valid = false;            // Wtb_ holds the bf16 fragments of the current W as it lies in Wt_ (unsmoothed; without the pending column scale)
	bool hb_valid = false;             // Hb_ holds the bf16 fragments of the current smoothed H (written by the H update)
	bool tri_gw_ready = false;         // Gw_raw_ / G_ describe the current W
	bool qx3_holds_g = false, qx3_holds_hht = false;   // qx3_ holds the split image of G_ / of the smoothed H H^T (k_smooth_gram)
	bool tri_scale_pending = false;    // W = Wt_ diag(d), d(c) = 1 / sqrt(staged sums in colsq_): the column normalisation of the last W update has not been folded into the panel
	bool tri_scale_from_gram = false;  // ... and its sums of squares are still to come out of the next Gram reduction (tri_prepare_w), into colsq_
	bool w_rows_stale = false;         // row-block sharded run with the fragment exchange: the fp32 rows of the other ranks' blocks in Wt_ are those of an earlier iteration
	bool tri_rows_cover = false;       // the last w_normalize_rows() covered every row of W
	bool gram_h_partials = false;      // gramH_part_ describes the current H
	bool online_stale = true;          // minibatch engines: online_A_ / online_B_ are set to W and 1 before the next step (the factors were set since the last one)

	constexpr void factors_touched() { online_stale = true; }      // set_factors / set_factors_device / randomize_factors, whichever factor: a minibatch engine starts again from A = W, B = 1
	// W set from outside: the panel is complete and normalised as the caller left it (hx3_valid: the split image of H goes with the W it was made beside)
	constexpr void w_set() { clear_w_core(); hx3_valid = false; wtb_valid = false; w_rows_stale = false; }
	constexpr void h_set() { hx3_valid = false; hb_valid = false; gram_h_partials = false; }
	// row-block sharded run: the blocks of every rank have been gathered into the panel (the fragments w_normalize_rows() left stay valid if it covered every row) /
	// the bf16 fragments of every rank's rows into Wtb_ (stale: the fp32 rows of the other ranks were not)
	constexpr void w_rows_replaced() { clear_w_core(); if (!tri_rows_cover) wtb_valid = false; }
	constexpr void w_fragments_gathered(bool stale) { clear_w_core(); wtb_valid = true; w_rows_stale = stale; }
	constexpr void v_replaced() { h_product_ahead = false; f64_product_ahead = false; }      // (finish_upload; H alone does not void the launches ahead: they read W and V)

private:
	constexpr void clear_w_core() {      // the W core: everything derived from the values of W alone, or enqueued with them
		kl_sw_ready = false; kl_scale_pending = false; fused_ready = false; w_pending = false; f32w_pending = false; f64_pending = false; f64_product_ahead = false;
		h_product_ahead = false; gram_w_ready = false; wx3_valid = false; tri_gw_ready = false; qx3_holds_g = false; tri_scale_pending = false; tri_scale_from_gram = false;
	}
};

// The table of the transitions, checked by the compiler: from the state with every flag set, `transition` leaves set exactly the flags listed (survive) or exactly
// the others (!survive: the list is what it clears).  The flags no transition writes, qx3_holds_hht and tri_rows_cover, survive all of them.
namespace panel_state_check {
using S = PanelState; using Flag = bool S::*;
constexpr Flag ALL[] = {&S::fused_ready, &S::w_pending, &S::h_product_ahead, &S::f32w_pending, &S::f64_pending, &S::f64_product_ahead, &S::kl_scale_pending, &S::kl_sw_ready,
                        &S::gram_w_ready, &S::wx3_valid, &S::hx3_valid, &S::wtb_valid, &S::hb_valid, &S::tri_gw_ready, &S::qx3_holds_g, &S::qx3_holds_hht, &S::tri_scale_pending,
                        &S::tri_scale_from_gram, &S::w_rows_stale, &S::tri_rows_cover, &S::gram_h_partials, &S::online_stale};
static_assert(sizeof(S) == sizeof(ALL) / sizeof(ALL[0]), "a flag of PanelState is missing from ALL");
template <typename F> constexpr bool leaves(F transition, bool survive, std::initializer_list<Flag> flags) {
	S s;
	for (Flag f : ALL) s.*f = true;
	transition(s);
	bool ok = true;
	for (Flag f : ALL) { bool listed = false; for (Flag k : flags) listed = listed || k == f; ok = ok && s.*f == (listed == survive); }
	return ok;
}
static_assert(leaves([](S& s) { s.factors_touched(); }, false, {}) && [] { S s; s.online_stale = false; s.factors_touched(); return s.online_stale; }(), "factors touched");
static_assert(leaves([](S& s) { s.w_set(); }, true, {&S::hb_valid, &S::qx3_holds_hht, &S::tri_rows_cover, &S::gram_h_partials, &S::online_stale}), "W set from outside");
static_assert(leaves([](S& s) { s.h_set(); }, false, {&S::hx3_valid, &S::hb_valid, &S::gram_h_partials}), "H set from outside: the W core survives, the launches ahead included");
static_assert(leaves([](S& s) { s.w_rows_replaced(); }, true, {&S::hx3_valid, &S::wtb_valid, &S::hb_valid, &S::qx3_holds_hht, &S::w_rows_stale, &S::tri_rows_cover,
              &S::gram_h_partials, &S::online_stale}), "W rows replaced, every row covered: the fragments survive");
static_assert(leaves([](S& s) { s.tri_rows_cover = false; s.w_rows_replaced(); }, true, {&S::hx3_valid, &S::hb_valid, &S::qx3_holds_hht, &S::w_rows_stale, &S::gram_h_partials,
              &S::online_stale}), "W rows replaced, not every row covered: the fragments go");
static_assert(leaves([](S& s) { s.w_fragments_gathered(true); }, true, {&S::hx3_valid, &S::wtb_valid, &S::hb_valid, &S::qx3_holds_hht, &S::w_rows_stale, &S::tri_rows_cover,
              &S::gram_h_partials, &S::online_stale}), "W fragments gathered(stale = true): w_rows_stale is the argument");
static_assert(leaves([](S& s) { s.v_replaced(); }, false, {&S::h_product_ahead, &S::f64_product_ahead}), "V replaced: only the two launches ahead go");
} // namespace panel_state_check

} // namespace nmfamd
