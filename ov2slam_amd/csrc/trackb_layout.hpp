// trackb_layout.hpp -- the ONE place that knows where things lie in the lock-step tracker's host-visible blocks (trackb.hip): the
// point block, the map block, the pose block, the epipolar I/O block, the filter's device-only index block, the three blocks of
// ov2_btracker_track_mono, the block of ov2_btracker_create_keyframe, the two blocks of the resident frame, the block of
// ov2_btracker_stereo_keyframe, the blocks of ov2_btracker_temporal_keyframe and the block of ov2_btracker_mono_init, each computed
// by one function of (batch, n_max) (stereo_keyframe and temporal_keyframe: and the grid's cells / the anchor table's rows).  Plain C++ (no HIP types, no context): trackb.hip includes it, tests/test_lockstep_layout.py compiles
// it alone with g++ and checks every offset.  `slots` below is batch x n_max; a section start is a multiple of 256 unless noted.
#pragma once
#include <stddef.h>
#include "stage.hpp"

#define BT_POSE_OUT_BYTES 168       // sizeof(PoseOut), sizeof(EpifOut), sizeof(FeKfHdr): trackb.hip asserts all three
#define BT_EPIF_OUT_BYTES 304
#define BT_KF_HDR_BYTES 120

// frames: row pitch and bytes of one item in the staging sets
static inline size_t bt_img_pitch(int w) { return up16((size_t)w); }
static inline size_t bt_img_bytes(int w, int h) { return up256(bt_img_pitch(w) * (size_t)h); }
// keyframe detection: [n 4 per item][current keypoints 8 per slot]
static inline size_t bt_det_in_bytes(int batch, int n_max) { return up256(4 * (size_t)batch) + 8 * (size_t)n_max * (size_t)batch; }

// The point block.  [n 4 per item][kps 8][prior 8][flag 1 per slot] go up (in_bytes; o_pri and o_flg follow their predecessor
// directly); [out 8][status 1 per slot (o_st follows o_out directly)][unpx 8][bv 24 per slot] come down.
struct BtPointLayout { size_t o_n, o_kps, o_pri, o_flg, in_bytes, o_out, o_st, o_unpx, o_bv, blk_bytes; };
static inline BtPointLayout bt_point_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    BtPointLayout L;
    L.o_n = 0; L.o_kps = up256(4 * B); L.o_pri = L.o_kps + 8 * slots; L.o_flg = L.o_pri + 8 * slots; L.in_bytes = up256(L.o_flg + slots);
    L.o_out = L.in_bytes; L.o_st = L.o_out + 8 * slots; L.o_unpx = up256(L.o_st + slots); L.o_bv = up256(L.o_unpx + 8 * slots);
    L.blk_bytes = L.o_bv + 24 * slots;
    return L;
}

// The map block: [items 16][Tcw 56 per item][wpt 24][is3d 1 per slot], all of it goes up.
struct BtMapLayout { size_t m_it, m_T, m_w, m_3d, map_bytes; };
static inline BtMapLayout bt_map_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    BtMapLayout L;
    L.m_it = 0; L.m_T = up256(16 * B); L.m_w = up256(L.m_T + 56 * B); L.m_3d = up256(L.m_w + 24 * slots);
    L.map_bytes = up256(L.m_3d + slots);
    return L;
}

// The pose block: [Twc 56][seed 8][flags 1 per item][scale 4 per slot] go up (q_in); [PoseOut 168][m, rows 8 per item]
// [removed 1 per slot] come down.
struct BtPoseLayout { size_t q_T, q_seed, q_fl, q_sc, q_in, q_out, q_ms, q_rm, pose_bytes; };
static inline BtPoseLayout bt_pose_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    BtPoseLayout L;
    L.q_T = 0; L.q_seed = up256(56 * B); L.q_fl = up256(L.q_seed + 8 * B); L.q_sc = up256(L.q_fl + B); L.q_in = up256(L.q_sc + 4 * slots);
    L.q_out = L.q_in; L.q_ms = up256(L.q_out + BT_POSE_OUT_BYTES * B); L.q_rm = up256(L.q_ms + 8 * B); L.pose_bytes = up256(L.q_rm + slots);
    return L;
}

// The epipolar blocks.  I/O block: [lmid 4 per slot][nbkfs 4][seed 8 per item] go up (e_in); [EpifOut 304][n_cur 4 per item]
// [removed 1][err 4][pair 4 per slot] come down.  Index block (device only): [FeKfHdr 120 per item][slot 4][rank 4 per slot (x_rank
// follows x_slot directly)].
struct BtEpiLayout { size_t e_lm, e_nk, e_sd, e_in, e_out, e_nc, e_rm, e_er, e_pc, epi_bytes, x_slot, x_rank, fx_bytes; };
static inline BtEpiLayout bt_epi_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    BtEpiLayout L;
    L.e_lm = 0; L.e_nk = up256(4 * slots); L.e_sd = up256(L.e_nk + 4 * B); L.e_in = up256(L.e_sd + 8 * B);
    L.e_out = L.e_in; L.e_nc = up256(L.e_out + BT_EPIF_OUT_BYTES * B); L.e_rm = up256(L.e_nc + 4 * B);
    L.e_er = up256(L.e_rm + slots); L.e_pc = up256(L.e_er + 4 * slots); L.epi_bytes = up256(L.e_pc + 4 * slots);
    L.x_slot = up256(BT_KF_HDR_BYTES * B); L.x_rank = L.x_slot + 4 * slots; L.fx_bytes = L.x_rank + 4 * slots;
    return L;
}

// The blocks of ov2_btracker_track_mono.  I/O block: [time 8][frame_id 4][localba 4 per item] go up (n_in); [predicted Twc 56]
// [state after apply 112][state after update 112][decision 48 (FKF_OUT_INTS ints)][n_cur 4][resynced 1 per item] come down.
// Resident block (device only, mirrored on the host): [Twc 56][ov2_motion_state 112][kf_time 8][kf_id, kf_nb3dkps, has_info, pad 16
// per item].  Work block (device only): [FkfItemD 176 per item][lmid 4][px 8][unpx 8][bv 24][is3d 1 per slot]: the frame
// checkNewKfReq sees, item b's at b x n_max.
#define BT_MOTION_STATE_BYTES 112   // sizeof(ov2_motion_state), sizeof(FkfItemD), 4 * FKF_OUT_INTS: trackb.hip asserts all three
#define BT_FKF_ITEM_BYTES 176
#define BT_KF_DEC_BYTES 48
struct BtMonoLayout {
    size_t n_tm, n_id, n_ba, n_in, n_pT, n_sa, n_su, n_dec, n_nc, n_rs, mono_bytes;
    size_t r_T, r_st, r_kt, r_ki, res_bytes;
    size_t w_it, w_lm, w_px, w_un, w_bv, w_3d, work_bytes;
};
static inline BtMonoLayout bt_mono_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    BtMonoLayout L;
    L.n_tm = 0; L.n_id = up256(8 * B); L.n_ba = up256(L.n_id + 4 * B); L.n_in = up256(L.n_ba + 4 * B);
    L.n_pT = L.n_in; L.n_sa = up256(L.n_pT + 56 * B); L.n_su = up256(L.n_sa + BT_MOTION_STATE_BYTES * B);
    L.n_dec = up256(L.n_su + BT_MOTION_STATE_BYTES * B); L.n_nc = up256(L.n_dec + BT_KF_DEC_BYTES * B); L.n_rs = up256(L.n_nc + 4 * B);
    L.mono_bytes = up256(L.n_rs + B);
    L.r_T = 0; L.r_st = up256(56 * B); L.r_kt = up256(L.r_st + BT_MOTION_STATE_BYTES * B); L.r_ki = up256(L.r_kt + 8 * B);
    L.res_bytes = up256(L.r_ki + 16 * B);
    L.w_it = 0; L.w_lm = up256(BT_FKF_ITEM_BYTES * B); L.w_px = up256(L.w_lm + 4 * slots); L.w_un = up256(L.w_px + 8 * slots);
    L.w_bv = up256(L.w_un + 8 * slots); L.w_3d = up256(L.w_bv + 24 * slots); L.work_bytes = up256(L.w_3d + slots);
    return L;
}

// The block of ov2_btracker_create_keyframe: one pinned host block and its device mirror at the same offsets, ONE copy up ([0, c_up))
// and ONE copy down ([c_io, c_down) with descriptors, [c_io, c_desc) without).
//   up only     [n 4][make_kf 1][nlmid 4][nkfid 4][time 8][Twc 56][quality 8 or fast_th 4, in 8 per item][is3d 1 per slot]
//   up and down [px 8][lmid 4 per slot]: the frame, the new points appended behind slot n on the device
//   down only   [record 32][SelectOut 56][FeKfHdr 120 per item][unpx 8][bv 24][colour 1][perm 4 (slot of the keyframe's i-th id) per
//               slot][desc 32][valid 1 per slot]
//   device only [skip 1][count 4 per item]: the detector's skip byte and the frame's size for computeKeypoint / BRIEF
#define BT_CKF_REC_BYTES 32          // sizeof(ov2_create_keyframe_result), sizeof(SelectOut): trackb.hip asserts both
#define BT_CKF_SO_BYTES 56
struct BtCkfLayout {
    size_t c_n, c_fl, c_nl, c_id, c_tm, c_T, c_par, c_3d, c_io, c_px, c_lm, c_up;
    size_t c_rec, c_so, c_hdr, c_un, c_bv, c_col, c_perm, c_desc, c_val, c_down;
    size_t w_skip, w_nb, dev_bytes;
};
static inline BtCkfLayout bt_ckf_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    StageCursor c(256);
    BtCkfLayout L;
    L.c_n = c.take(4 * B); L.c_fl = c.take(B); L.c_nl = c.take(4 * B); L.c_id = c.take(4 * B); L.c_tm = c.take(8 * B); L.c_T = c.take(56 * B);
    L.c_par = c.take(8 * B); L.c_3d = c.take(slots);
    L.c_io = L.c_px = c.take(8 * slots); L.c_lm = c.take(4 * slots); L.c_up = c.off;
    L.c_rec = c.take(BT_CKF_REC_BYTES * B); L.c_so = c.take(BT_CKF_SO_BYTES * B); L.c_hdr = c.take(BT_KF_HDR_BYTES * B);
    L.c_un = c.take(8 * slots); L.c_bv = c.take(24 * slots); L.c_col = c.take(slots); L.c_perm = c.take(4 * slots);
    L.c_desc = c.take(32 * slots); L.c_val = c.take(slots); L.c_down = c.off;
    L.w_skip = c.take(B); L.w_nb = c.take(4 * B); L.dev_bytes = c.off;
    return L;
}

// The resident frame (ov2_btracker_set_frame / _update_frame / _track_mono_resident): the current frame of every item, kept on the
// device from step to step.  ITEM-MAJOR, so that the frames of items [b0, b1) are one contiguous range (one copy per direction):
//   one item    [n 4, padded to 16][px 8][lmid 4][is3d 1][wpt 24 per slot], f_item bytes (a multiple of 256)
//   one buffer  batch items; the block holds TWO buffers (a step reads an item's frame from one and writes the next frame into the
//               other; which one is current is kept per item on the host and travels as one byte per item)
// The pinned host mirror has the same layout.  The control block of a call (pinned, and its device mirror at the same offsets):
//   up    [sel 1][n_ops 4][first op 4 per item][ops 32 per slot, PACKED: item b's list starts at its first op]   (u_up at capacity;
//         an update sends [0, u_ops + 32 x the ops of the call), a step or a create_keyframe call [0, u_nop) only)
//   down  [record 24 per item]
#define BT_RES_OP_BYTES 32           // sizeof(ov2_resident_op), sizeof(ov2_resident_update_result): trackb.hip asserts both
#define BT_RES_REC_BYTES 24
struct BtResLayout {
    size_t f_n, f_px, f_lm, f_3d, f_w, f_item, buf_bytes, frame_bytes;
    size_t u_sel, u_nop, u_off, u_ops, u_up, u_rec, ctl_bytes;
};
static inline BtResLayout bt_res_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, nm = (size_t)n_max, slots = nm * B;
    BtResLayout L;
    StageCursor f(16);
    L.f_n = f.take(4); L.f_px = f.take(8 * nm); L.f_lm = f.take(4 * nm); L.f_3d = f.take(nm); L.f_w = f.take(24 * nm);
    L.f_item = up256(f.off); L.buf_bytes = L.f_item * B; L.frame_bytes = 2 * L.buf_bytes;
    StageCursor c(256);
    L.u_sel = c.take(B); L.u_nop = c.take(4 * B); L.u_off = c.take(4 * B); L.u_ops = c.take(BT_RES_OP_BYTES * slots);
    L.u_up = c.off; L.u_rec = c.take(BT_RES_REC_BYTES * B); L.ctl_bytes = c.off;
    return L;
}

// The block of ov2_btracker_stereo_keyframe (f22): one pinned host block [0, s_down) and its device mirror at the same offsets,
// ONE copy up ([0, s_up)) and ONE copy down ([s_io, s_down)); behind s_down the device-only work ranges of the kernels between.
// `cells` is the grid of Frame::getSurroundingKeypoints (0 for a rectified pair: no grid).
//   up only     [act 1 per item]: 1 where the item is OV2_SKF_DONE
//   down only   [record 32 per item][right_px 8][wpt 24][invdepth 8][stereo_ok 1][tri_status 1 per slot]
//   device only [PriItemD 16][tri item 16][Tcw 56][Twc 56][count 4 per item]
//               [px 8][unpx 8][bv 24][frame wpt 24][pts_top 8][prior 8][LK out 8][gate runpx 8][runpx 8][rbv 24][src 4][sad x 4]
//               [sad err 4][gate err 4][state 1][has_prior 1][skip 1][flag 1][LK status 1][gate ok 1][is_stereo 1 per slot]
//               [cell_start 4 per cell + 1 per item][cell_kp 4 per slot]
#define BT_SKF_REC_BYTES 32          // sizeof(ov2_stereo_keyframe_result): trackb.hip asserts it
struct BtSkfLayout {
    size_t s_act, s_up, s_io, s_rec, s_rpx, s_wpt, s_inv, s_sok, s_tst, s_down;
    size_t w_pit, w_tit, w_Tcw, w_Twc, w_nd;
    size_t w_px, w_un, w_bv, w_fw, w_top, w_pri, w_out, w_gru, w_ru, w_rbv, w_src, w_sx, w_l1, w_err;
    size_t w_st, w_hp, w_sk, w_fl, w_lk, w_ok, w_is, w_cs, w_ck, dev_bytes;
};
static inline BtSkfLayout bt_skf_layout(int batch, int n_max, int cells)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    StageCursor c(256);
    BtSkfLayout L;
    L.s_act = c.take(B); L.s_up = c.off;
    L.s_io = L.s_rec = c.take(BT_SKF_REC_BYTES * B); L.s_rpx = c.take(8 * slots); L.s_wpt = c.take(24 * slots); L.s_inv = c.take(8 * slots);
    L.s_sok = c.take(slots); L.s_tst = c.take(slots); L.s_down = c.off;
    L.w_pit = c.take(16 * B); L.w_tit = c.take(16 * B); L.w_Tcw = c.take(56 * B); L.w_Twc = c.take(56 * B); L.w_nd = c.take(4 * B);
    L.w_px = c.take(8 * slots); L.w_un = c.take(8 * slots); L.w_bv = c.take(24 * slots); L.w_fw = c.take(24 * slots);
    L.w_top = c.take(8 * slots); L.w_pri = c.take(8 * slots); L.w_out = c.take(8 * slots); L.w_gru = c.take(8 * slots);
    L.w_ru = c.take(8 * slots); L.w_rbv = c.take(24 * slots); L.w_src = c.take(4 * slots); L.w_sx = c.take(4 * slots);
    L.w_l1 = c.take(4 * slots); L.w_err = c.take(4 * slots);
    L.w_st = c.take(slots); L.w_hp = c.take(slots); L.w_sk = c.take(slots); L.w_fl = c.take(slots); L.w_lk = c.take(slots);
    L.w_ok = c.take(slots); L.w_is = c.take(slots);
    L.w_cs = c.take(4 * ((size_t)cells + 1) * B); L.w_ck = c.take(4 * slots); L.dev_bytes = c.off;
    return L;
}

// The blocks of ov2_btracker_temporal_keyframe (f23).  The ANCHOR TABLE: per item the first observing keyframe of every keypoint of
// its latest keyframe, ITEM-MAJOR and double-buffered like the resident frame (a call reads an item's table from one buffer and
// writes the next one into the other; which one is current is kept per item on the host and travels as one byte per item), with a
// pinned host mirror of the same layout:
//   one item    [n 4, padded to 16][lmid 4][row 4][unpx 8][bv 24 per slot, ascending by lmid]
//               [n_rows 4, padded to 16][kfid 4][Twc 56][Tcw 56 per row, ascending by kfid], a_item bytes (a multiple of 256)
// The control block of a call: one pinned host block [0, t_down) and its device mirror at the same offsets, ONE copy up ([0, t_up))
// and ONE copy down ([t_io, t_down)); behind t_down the device-only work ranges of the kernels.
//   up only     [act 1][asel 1 per item]: 1 where the item is asked and its frame is its keyframe; the buffer of its current table
//   down only   [record 32 per item][wpt 24][invdepth 8][src_kfid 4][tri_status 1 per slot]
//   device only [tri item 16][Twc 56][overflow 4 per item][source rows 112 per row (Twc, Tcw)]
//               [unpx 8][bv 24][src_unpx 8][src_bv 24][src 4][is_stereo 1 per slot]
// The block of ov2_btracker_set_anchor_poses (pinned, and its device mirror): [item 4][kfid 4][Twc 56 per triple], batch x n_src_max
// triples at the most.
#define BT_TKF_REC_BYTES 32          // sizeof(ov2_temporal_keyframe_result): trackb.hip asserts it
struct BtTkfLayout {
    size_t a_n, a_lm, a_row, a_un, a_bv, a_nr, a_kf, a_Twc, a_Tcw, a_item, buf_bytes, anchor_bytes;
    size_t t_act, t_sel, t_up, t_io, t_rec, t_wpt, t_inv, t_skf, t_tst, t_down;
    size_t w_tit, w_Twc, w_ovf, w_srcT, w_un, w_bv, w_sun, w_sbv, w_src, w_is, dev_bytes;
    size_t p_item, p_kfid, p_Twc, pose_bytes;
};
static inline BtTkfLayout bt_tkf_layout(int batch, int n_max, int n_src_max)
{
    const size_t B = (size_t)batch, nm = (size_t)n_max, ns = (size_t)n_src_max, slots = nm * B, rows = ns * B;
    BtTkfLayout L;
    StageCursor f(16);
    L.a_n = f.take(4); L.a_lm = f.take(4 * nm); L.a_row = f.take(4 * nm); L.a_un = f.take(8 * nm); L.a_bv = f.take(24 * nm);
    L.a_nr = f.take(4); L.a_kf = f.take(4 * ns); L.a_Twc = f.take(56 * ns); L.a_Tcw = f.take(56 * ns);
    L.a_item = up256(f.off); L.buf_bytes = L.a_item * B; L.anchor_bytes = 2 * L.buf_bytes;
    StageCursor c(256);
    L.t_act = c.take(B); L.t_sel = c.take(B); L.t_up = c.off;
    L.t_io = L.t_rec = c.take(BT_TKF_REC_BYTES * B); L.t_wpt = c.take(24 * slots); L.t_inv = c.take(8 * slots); L.t_skf = c.take(4 * slots);
    L.t_tst = c.take(slots); L.t_down = c.off;
    L.w_tit = c.take(16 * B); L.w_Twc = c.take(56 * B); L.w_ovf = c.take(4 * B); L.w_srcT = c.take(112 * rows);
    L.w_un = c.take(8 * slots); L.w_bv = c.take(24 * slots); L.w_sun = c.take(8 * slots); L.w_sbv = c.take(24 * slots);
    L.w_src = c.take(4 * slots); L.w_is = c.take(slots); L.dev_bytes = c.off;
    StageCursor q(256);
    L.p_item = q.take(4 * rows); L.p_kfid = q.take(4 * rows); L.p_Twc = q.take(56 * rows); L.pose_bytes = q.off;
    return L;
}

// The block of ov2_btracker_mono_init (f25): one pinned host block [0, i_down) and its device mirror at the same offsets, ONE copy up
// ([0, i_up)) and ONE copy down ([i_io, i_down)); behind i_down the device-only ranges: what k_minit_input leaves for
// Frame::computeKeypoint, then (at w_chain) the chain's own block -- monoinit_dev.hpp: MinitLayout at capacity, batch x n_max slots and
// batch x n_rows rows, so its size follows the rows of the call and the device half is grown when a call asks for more.
//   up only     [act 1][seed 8 per item]: 1 where the item is requested and has a resident keyframe with its info
//   down only   [record 224 per item][removed 1 per slot]
//   device only [count 4 per item][px 8 per slot][the chain's block]
#define BT_MINIT_REC_BYTES 224       // sizeof(MinitOut): trackb.hip asserts it
struct BtMinitLayout { size_t i_act, i_seed, i_up, i_io, i_rec, i_rm, i_down, w_nd, w_px, w_chain; };
static inline BtMinitLayout bt_minit_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, slots = (size_t)n_max * B;
    StageCursor c(256);
    BtMinitLayout L;
    L.i_act = c.take(B); L.i_seed = c.take(8 * B); L.i_up = c.off;
    L.i_io = L.i_rec = c.take(BT_MINIT_REC_BYTES * B); L.i_rm = c.take(slots); L.i_down = c.off;
    L.w_nd = c.take(4 * B); L.w_px = c.take(8 * slots); L.w_chain = c.off;
    return L;
}

// The keyframe store of the from-keyframe mode (ov2_btracker_set_track_from_keyframe).  The KEYFRAME-PX TABLE: per item the distorted
// px of every keypoint its keyframe had when it was created, ITEM-MAJOR like the resident frame, with a pinned host mirror of the same
// layout.  A snapshot that is only ever looked up by lmid: membership is the resident keyframe's own list.
//   one item    [n 4, padded to 16][lmid 4][px 8 per slot, ascending by lmid], k_item bytes (a multiple of 256)
// Behind the table, in the same block: [adopt flag 1 per item] (pinned too: ov2_btracker_adopt_keyframe_pyramid sends it up) and,
// device only, the source point of every slot of a step [src 8 per slot] (k_kf_join writes it, the tracking kernel reads it).
struct BtKfPxLayout { size_t k_n, k_lm, k_px, k_item, table_bytes, k_flag, host_bytes, w_src, dev_bytes; };
static inline BtKfPxLayout bt_kfpx_layout(int batch, int n_max)
{
    const size_t B = (size_t)batch, nm = (size_t)n_max, slots = nm * B;
    BtKfPxLayout L;
    StageCursor f(16);
    L.k_n = f.take(4); L.k_lm = f.take(4 * nm); L.k_px = f.take(8 * nm);
    L.k_item = up256(f.off); L.table_bytes = L.k_item * B;
    L.k_flag = L.table_bytes; L.host_bytes = up256(L.k_flag + B);
    L.w_src = L.host_bytes; L.dev_bytes = up256(L.w_src + 8 * slots);
    return L;
}
