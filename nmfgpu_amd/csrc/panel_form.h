// panel_form.h -- which kernel of kernels_wide.hip the last panel-update launch of this thread went to: test access (nmfamd_op_panel_update_last_form), so that a
// launcher's choice between forms that return the same values can be asserted (docs/PANEL_UPDATE.md).  One thread-local word written per launch on the host.
#pragma once

namespace nmfamd {

enum PanelForm {
	PANEL_FORM_OTHER = 0,        // a kernel outside kernels_wide.hip (the generic one, the fp64 ones, k_panel_update64_f32)
	PANEL_FORM_LDS64 = 1,        // k_panel_update64_lds_f32
	PANEL_FORM_WIDE32 = 2,       // k_panel_update_wide_f32, 32 rows per workgroup
	PANEL_FORM_WIDE32_FUSED = 3, // ... its FX instantiation
	PANEL_FORM_ROWS128 = 4,      // k_panel_update_rows_mu, 128 rows per workgroup
	PANEL_FORM_WIDE64 = 5,       // k_panel_update_wide64_mu, 64 rows per workgroup
};
int panel_update_last_form();
void panel_update_reset_form();

} // namespace nmfamd
