// kltkf_dev.hpp -- what trackb.hip / trackb_keyframe.hip and kltkf.hip share for the from-keyframe mode of the lock-step tracker
// (VisualFrontEnd::kltTrackingFromKF, src/visual_front_end.cpp:278-442): the device view of the keyframe-px table
// (trackb_layout.hpp: BtKfPxLayout), the pointers of the three launches, and the launchers.
//   k_kfpx_install   behind k_ckf_install: the px table of every CREATED item from the create-keyframe block, and its adopt flag
//   k_kfpyr_adopt    the current pyramid item of every flagged item into the keyframe store, one streaming copy
//   k_kf_join        behind k_prior_frame: per slot the keyframe's px as the source point, or the skip flag
#pragma once
#include "common.hpp"
#include "frameepi_dev.hpp"

// the px table: item b starts at base + b * k_item
struct KfPxTable { uint8_t *base; size_t k_item, k_lm, k_px; int n_max; };

struct KfPxInstallArgs {
    KfPxTable tab;
    const uint8_t *make_kf;                             // the call's request byte per item
    const ov2_create_keyframe_result *rec;              // action and n_kf as k_ckf_install left them
    const float2 *px; const int *lmid, *perm;           // the new frame, and the slot of the keyframe's i-th id
    uint8_t *adopt;                                     // out: 1 where the item's pyramid is to be adopted
};

struct KfJoinArgs {
    KfPxTable tab;
    const int *n_dev, *lmid;                            // the frame: its size per item, n_max ids per item
    const FeKfHdr *hdr; const int *kf_lmid;             // the resident keyframe: n_kf and its ascending ids
    const float2 *kps;                                  // the frame's current px
    float2 *src; uint8_t *flags;                        // out: the source point; flag 2 replaces k_prior_frame's where the slot is skipped
};

int ov2_launch_kfpx_install(hipStream_t s, const KfPxInstallArgs &a, int n_active);
// items [0, n_active) of `cur` whose flag byte is set, every level with its borders (the whole item stride), into `store`
int ov2_launch_kfpyr_adopt(hipStream_t s, const PyrDesc &cur, const PyrDesc &store, const uint8_t *flag_d, int n_active);
int ov2_launch_kf_join(hipStream_t s, const KfJoinArgs &a, int n_active);

// The 33 % rule of kltTrackingFromKF (:395-400) over the n results of one frame, the sibling of ov2_apply_p3p_rule.  flags: what
// k_kf_join left (bit 0 entered the prior pass, bit 1 skipped).  When fewer than 33 % of the prior-pass slots are good, `vpriors =
// vkps` resets EVERY prior of the second call: each slot whose result comes from that call (no prior, or status bit 1) is run again
// from the keyframe's item to the current one on the full pyramid with prior = source = the keyframe's px; good prior-pass tracks stay.
// lmid: the frame's ids; tab_lmid / tab_px: the item's px table (n_tab entries, ascending), where a re-run slot's source point is.
struct KfRuleFrame { const int *lmid; const int *tab_lmid; const float *tab_px; int n_tab; const uint8_t *flags; int n; float *out_xy;
                     uint8_t *status; float *unpx; double *bv; };
int ov2_apply_p3p_rule_kf(ov2_ctx *ctx, const ov2_tracker_config &cfg, const ov2_pyr *kf, const ov2_pyr *cur, const KpCalib *calib,
                          const KfRuleFrame &f, int *p3p_req);
