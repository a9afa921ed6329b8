// rmpc_desc.hpp -- from the descriptor of the C ABI (rmpc_desc, rmpc.h) to what the kernels read: the checks of
// a descriptor, the model (DevModel), the row tables (DevTables) and the source text of a generated view.  Host
// C++ only, no HIP call and no kernel file: rmpc_host.hip includes it, and so does the sanitizer harness
// tests/host/host_sweep.cpp.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rmpc_model.hpp"

namespace rmpc {

// rmpc_desc.ls_max <= 0 means this many step halvings.  It is the solver's kLsMax (rmpc_solver.hpp), which this
// header does not see; rmpc_host.hip sees both and asserts that they agree.
constexpr int kDescLsMax = 25;

/* a descriptor of this version, or of 0.2.0 (the struct without the xrow_* arrays at its end: no row-described modules) */
static bool take_desc(const rmpc_desc *in, rmpc_desc &full) {
  if (!in) return false;
  const int old_size = (int)offsetof(rmpc_desc, n_xrows);
  if (in->struct_size != (int)sizeof(rmpc_desc) && in->struct_size != old_size) return false;
  memset(&full, 0, sizeof full);
  memcpy(&full, in, (size_t)in->struct_size);
  full.struct_size = (int)sizeof(rmpc_desc);
  return true;
}

// Row tables in device memory (DevTables): kinematic slots with their FK rows, and the
// single-variable rows grouped by variable.
static int build_tables(const rmpc_desc &d, const DevModel &M, DevTables &T, std::string &err) {
  memset(&T, 0, sizeof T);
  for (int s = 0; s < kMaxSlots; s++) { T.slot_fa[s] = -1; T.slot_fb[s] = -1; }
  for (int j = 0; j < RMPC_NV_MAX; j++)
    for (int u = 0; u < kVarRows; u++) { T.v_row[j][u] = -1; T.v_poff[j][u] = -1; T.v_mod[j][u] = -1; }
  auto slot_of = [&](int fa, int fb) -> int {
    for (int s = 0; s < T.nslots; s++)
      if (T.slot_fa[s] == fa && T.slot_fb[s] == fb) return s;
    if (T.nslots >= kMaxSlots) return -1;
    T.slot_fa[T.nslots] = fa; T.slot_fb[T.nslots] = fb;
    return T.nslots++;
  };
  if (d.has_goal && slot_of(d.end_frame, -1) != 0) { err = "slot table"; return -1; }
  // FK rows with their slots, then sorted by slot
  struct FkRow { int row, kind, obst, mod, first, idx, slot; };
  std::vector<FkRow> rows;
  for (int i = 0; i < M.nh; i++) {
    if (M.row_kind[i] == ROW_SINGLE) continue;
    const int fb = (M.row_kind[i] == ROW_SELF) ? M.row_b[i] : -1;
    const int s = slot_of(M.row_a[i], fb);
    if (s < 0) { err = "more than 4 distinct collision points (links / link pairs / end link)"; return -1; }
    rows.push_back({i, M.row_kind[i], M.row_kind[i] == ROW_SELF ? 0 : M.row_b[i], M.row_mod[i],
                    i == M.mod_row0[M.row_mod[i]] ? 1 : 0, M.row_fk[i], s});
  }
  if ((int)rows.size() > kMaxFkRows) { err = "too many distance rows"; return -1; }
  int r = 0;
  for (int s = 0; s < kMaxSlots; s++) {
    T.slot_row_begin[s] = r;
    for (const FkRow &fr : rows)
      if (fr.slot == s) {
        T.fk_row[r] = fr.row; T.fk_kind[r] = fr.kind; T.fk_obst[r] = fr.obst;
        T.fk_mod[r] = fr.mod; T.fk_first[r] = fr.first; T.fk_idx[r] = fr.idx;
        r++;
      }
  }
  T.slot_row_begin[kMaxSlots] = r;
  T.nfkrows = r;
  // single-variable rows
  auto add_var_row = [&](int var, int row, int sgn, int poff, double val, int soft, int mod, int firstrow) -> bool {
    for (int u = 0; u < kVarRows; u++)
      if (T.v_row[var][u] < 0) {
        T.v_row[var][u] = row; T.v_sgn[var][u] = sgn; T.v_poff[var][u] = poff;
        T.v_val[var][u] = val; T.v_soft[var][u] = soft; T.v_mod[var][u] = mod;
        T.v_first[var][u] = firstrow;
        return true;
      }
    return false;
  };
  bool ok = true;
  for (int i = 0; i < M.nh && ok; i++)
    if (M.row_kind[i] == ROW_SINGLE)
      ok = add_var_row(M.row_a[i], i, M.row_b[i], M.row_poff[i], 0.0, 1, M.row_mod[i], i == M.mod_row0[M.row_mod[i]] ? 1 : 0);
  int i = M.nh;
  for (int q = 0; q < M.nlb && ok; q++, i++) ok = add_var_row(M.lb_var[q], i, +1, -1, M.lb_val[q], 0, -1, 0);
  for (int q = 0; q < M.nub && ok; q++, i++) ok = add_var_row(M.ub_var[q], i, -1, -1, M.ub_val[q], 0, -1, 0);
  if (!ok) { err = "more than 4 limit / bound rows on one variable"; return -1; }
  // packed copies (fused arm kernel)
  for (int j = 0; j < RMPC_NV_MAX; j++)
    for (int u = 0; u < kVarRows; u++) {
      int w = 0;
      if (T.v_row[j][u] >= 0 && T.v_row[j][u] < 256 && T.v_poff[j][u] < 65536) {
        w = T.v_row[j][u] | (1 << 8) | ((T.v_sgn[j][u] < 0 ? 1 : 0) << 9) | ((T.v_first[j][u] ? 1 : 0) << 10) |
            ((T.v_poff[j][u] >= 0 ? 1 : 0) << 11) | ((T.v_mod[j][u] >= 0 ? T.v_mod[j][u] & 7 : 0) << 12) |
            ((T.v_poff[j][u] >= 0 ? T.v_poff[j][u] : 0) << 16);
      }
      T.v_desc[j][u] = w;
    }
  for (int q = 0; q < T.nfkrows; q++)
    T.fk_desc[q] = (T.fk_row[q] & 255) | ((T.fk_kind[q] & 3) << 8) | ((T.fk_obst[q] & 63) << 10) | ((T.fk_mod[q] & 7) << 16) |
                   ((T.fk_first[q] ? 1 : 0) << 19) | ((T.fk_idx[q] & 63) << 20);
  T.slot_rows_max = 0;
  for (int s = 0; s < kMaxSlots; s++)
    if (T.slot_row_begin[s + 1] - T.slot_row_begin[s] > T.slot_rows_max) T.slot_rows_max = T.slot_row_begin[s + 1] - T.slot_row_begin[s];
  return 0;
}

static int build_model(const rmpc_desc &d, DevModel &M, std::string &err) {
  memset(&M, 0, sizeof M);
  M.robot = d.robot; M.N = d.N; M.n = d.n; M.nx = d.nx; M.nu = d.nu; M.ns = d.ns;
  M.nv = d.nx + d.ns + d.nu; M.nw = d.ns + d.nu; M.npar = d.npar; M.dt = d.dt;
  if (d.N < 1 || d.N > 1000) { err = "horizon out of range"; return -1; }
  if (d.n_joints < 1 || d.n_joints > RMPC_MAX_JOINTS) { err = "n_joints out of range"; return -1; }
  if (d.ns != 0 && d.ns != 1) { err = "ns must be 0 or 1"; return -1; }
  if (d.robot == RMPC_ROBOT_CHAIN) {
    if (d.nx != 2 * d.n || d.nu != d.n) { err = "holonomic chain needs nx = 2n, nu = n"; return -1; }
    if (d.n_joints != d.n) { err = "chain with fixed joints between root and end link is not supported"; return -1; }
    for (int j = 0; j < d.n_joints; j++)
      if (d.joint_type[j] == RMPC_JOINT_FIXED || d.joint_dof[j] != j) { err = "chain joints must all be actuated, in order"; return -1; }
  } else if (d.robot == RMPC_ROBOT_DIFFDRIVE) {
    if (d.n != 3 || d.nx != 8 || d.nu != 2) { err = "diff-drive needs n = 3, nx = 8, nu = 2 (fk.n() == 0)"; return -1; }
    for (int j = 0; j < d.n_joints; j++)
      if (d.joint_type[j] != RMPC_JOINT_FIXED) { err = "diff-drive chain must consist of fixed joints"; return -1; }
  } else { err = "unknown robot kind"; return -1; }
  if (d.n_joints < 1 || d.n_joints > RMPC_MAX_JOINTS) { err = "n_joints out of range"; return -1; }
  if (M.nv > RMPC_NV_MAX) { err = "nvar too large"; return -1; }
  M.n_modules = d.n_modules; M.nobst = d.nobst; M.end_frame = d.end_frame; M.n_joints = d.n_joints;
  if (d.n_modules < 0 || d.n_modules > RMPC_MAX_MODULES) { err = "n_modules out of range"; return -1; }
  if (d.n_xrows < 0 || d.n_xrows > RMPC_MAX_XROWS) { err = "n_xrows out of range"; return -1; }
  for (int r = 0; r < d.n_xrows; r++)
    if (d.xrow_mod[r] < 0 || d.xrow_mod[r] >= d.n_modules || d.module_kind[d.xrow_mod[r]] != RMPC_MOD_ROWS) { err = "row description: xrow_mod must name a module of kind RMPC_MOD_ROWS"; return -1; }
  if (d.n_links < 0 || d.n_links > RMPC_MAX_LINKS || d.n_pairs < 0 || d.n_pairs > RMPC_MAX_PAIRS) { err = "links/pairs out of range"; return -1; }
  auto frame_ok = [&](int f) { return f >= 0 && f < d.n_joints; };
  if (!frame_ok(d.end_frame)) { err = "end_frame out of range"; return -1; }
  for (int j = 0; j < d.n_joints; j++) {
    M.joint_type[j] = d.joint_type[j];
    for (int c = 0; c < 3; c++) { M.joint_xyz[j][c] = d.joint_xyz[j][c]; M.joint_axis[j][c] = d.joint_axis[j][c]; }
    for (int c = 0; c < 9; c++) M.joint_rot[j][c] = d.joint_rot[j][c];
  }
  if (d.robot == RMPC_ROBOT_DIFFDRIVE) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
    for (int j = 0; j < d.n_joints; j++) {
      const double *t = d.joint_xyz[j];
      for (int r = 0; r < 3; r++) o[r] += R[3 * r] * t[0] + R[3 * r + 1] * t[1] + R[3 * r + 2] * t[2];
      double Rn[9];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
          Rn[3 * r + c] = R[3 * r] * d.joint_rot[j][c] + R[3 * r + 1] * d.joint_rot[j][3 + c] + R[3 * r + 2] * d.joint_rot[j][6 + c];
      memcpy(R, Rn, sizeof R);
      for (int c = 0; c < 3; c++) M.dd_off[j][c] = o[c];
    }
  }
  M.off_r_body = d.off_r_body; M.off_obst = d.off_obst; M.off_lin = d.off_lin; M.off_wu = d.off_wu;
  M.off_goal = d.off_goal; M.off_wgoal = d.off_wgoal; M.off_wconstr = d.off_wconstr; M.off_ws = d.off_ws;
  M.has_goal = d.has_goal; M.has_avoid = d.has_avoid;
  auto off_ok = [&](int off, int len) { return off >= 0 && off + len <= d.npar; };
  if (!off_ok(d.off_wu, d.nu)) { err = "off_wu"; return -1; }
  if (d.ns && !off_ok(d.off_ws, 1)) { err = "off_ws"; return -1; }
  if (d.has_goal && (!off_ok(d.off_goal, 3) || !off_ok(d.off_wgoal, 3))) { err = "goal offsets"; return -1; }
  if (d.has_avoid && !off_ok(d.off_wconstr, d.n_modules)) { err = "off_wconstr"; return -1; }
  // general rows in module order
  int row = 0, nfk = 0;
  for (int mi = 0; mi < d.n_modules; mi++) {
    M.mod_kind[mi] = d.module_kind[mi];
    M.mod_row0[mi] = row;
    auto push = [&](int kind, int a, int bb, int poff, bool fk) -> bool {
      if (row >= kMaxRows) return false;
      M.row_kind[row] = (int8_t)kind; M.row_a[row] = (int8_t)a; M.row_b[row] = (int8_t)bb;
      M.row_poff[row] = poff; M.row_fk[row] = fk ? (int8_t)nfk++ : (int8_t)-1; M.row_mod[row] = (int8_t)mi;
      row++;
      return true;
    };
    bool ok = true;
    switch (d.module_kind[mi]) {
      case RMPC_MOD_RADIAL:
        if (!off_ok(d.off_r_body, 1) || !off_ok(d.off_obst, 4 * d.nobst)) { err = "radial offsets"; return -1; }
        for (int l = 0; l < d.n_links && ok; l++) {
          if (!frame_ok(d.link_frame[l])) { err = "link frame"; return -1; }
          for (int i = 0; i < d.nobst && ok; i++) ok = push(ROW_RADIAL, d.link_frame[l], i, 0, true);
        }
        break;
      case RMPC_MOD_LINEAR:
        if (!off_ok(d.off_r_body, 1) || !off_ok(d.off_lin, 4 * d.nobst)) { err = "linear offsets"; return -1; }
        for (int l = 0; l < d.n_links && ok; l++) {
          if (!frame_ok(d.link_frame[l])) { err = "link frame"; return -1; }
          for (int i = 0; i < d.nobst && ok; i++) ok = push(ROW_LINEAR, d.link_frame[l], i, 0, true);
        }
        break;
      case RMPC_MOD_SELFCOLLISION:
        if (d.n_pairs > 0 && !off_ok(d.off_r_body, 1)) { err = "self collision offsets"; return -1; }
        for (int pi = 0; pi < d.n_pairs && ok; pi++) {
          if (!frame_ok(d.pair_frame[pi][0]) || !frame_ok(d.pair_frame[pi][1])) { err = "pair frame"; return -1; }
          ok = push(ROW_SELF, d.pair_frame[pi][0], d.pair_frame[pi][1], 0, true);
        }
        break;
      case RMPC_MOD_JOINTLIMIT:
        if (!off_ok(d.off_lower, d.n) || !off_ok(d.off_upper, d.n)) { err = "joint limit offsets"; return -1; }
        for (int j = 0; j < d.n && ok; j++) {
          ok = push(ROW_SINGLE, j, +1, d.off_lower + j, false);
          ok = ok && push(ROW_SINGLE, j, -1, d.off_upper + j, false);
        }
        break;
      case RMPC_MOD_VELLIMIT:
        if (!off_ok(d.off_lower_vel, 2) || !off_ok(d.off_upper_vel, 2)) { err = "velocity limit offsets"; return -1; }
        for (int j = 0; j < 2 && ok; j++) {
          ok = push(ROW_SINGLE, d.nx - 2 + j, +1, d.off_lower_vel + j, false);
          ok = ok && push(ROW_SINGLE, d.nx - 2 + j, -1, d.off_upper_vel + j, false);
        }
        break;
      case RMPC_MOD_INPUTLIMIT:
        if (!off_ok(d.off_lower_u, d.nu) || !off_ok(d.off_upper_u, d.nu)) { err = "input limit offsets"; return -1; }
        for (int j = 0; j < d.nu && ok; j++) {
          ok = push(ROW_SINGLE, d.nx + d.ns + j, +1, d.off_lower_u + j, false);
          ok = ok && push(ROW_SINGLE, d.nx + d.ns + j, -1, d.off_upper_u + j, false);
        }
        break;
      case RMPC_MOD_ROWS: {
        // a module given as row descriptions (rmpc.h): variants of the six kinds through the same row tables
        int on_x = 0, on_u = 0;
        for (int r = 0; r < d.n_xrows && ok; r++) {
          if (d.xrow_mod[r] != mi) continue;
          const int a = d.xrow_a[r], b = d.xrow_b[r], po = d.xrow_poff[r];
          switch (d.xrow_kind[r]) {
            case RMPC_ROW_RADIAL:
            case RMPC_ROW_LINEAR: {
              const bool radial = d.xrow_kind[r] == RMPC_ROW_RADIAL;
              int &base = radial ? M.off_obst : M.off_lin;
              if (!frame_ok(a)) { err = "row description: frame"; return -1; }
              if (!off_ok(d.off_r_body, 1) || !off_ok(po, 4)) { err = "row description: parameter offsets"; return -1; }
              if (base < 0) base = po;   // (no module of the kind: the list starts at the first described row)
              if (po < base || (po - base) % 4 != 0 || (po - base) / 4 > 63) {
                err = "row description: a sphere / plane must lie a multiple of 4 (at most 252) parameters behind the obstacle / plane list";
                return -1;
              }
              ok = push(radial ? ROW_RADIAL : ROW_LINEAR, a, (po - base) / 4, 0, true);
              on_x++;
              break;
            }
            case RMPC_ROW_SELF:
              if (!frame_ok(a) || !frame_ok(b) || a == b) { err = "row description: pair frames"; return -1; }
              if (!off_ok(d.off_r_body, 1)) { err = "row description: r_body"; return -1; }
              ok = push(ROW_SELF, a, b, 0, true);
              on_x++;
              break;
            case RMPC_ROW_VAR:
              if (a < 0 || a >= M.nv || (d.ns && a == d.nx)) { err = "row description: variable"; return -1; }
              if (b != 1 && b != -1) { err = "row description: sign must be +1 or -1"; return -1; }
              if (!off_ok(po, 1)) { err = "row description: limit offset"; return -1; }
              ok = push(ROW_SINGLE, a, b, po, false);
              (a < d.nx ? on_x : on_u)++;
              break;
            default:
              err = "row description: unknown row kind";
              return -1;
          }
        }
        if (on_x && on_u) { err = "row description: the rows of a module must all be on states or all on inputs"; return -1; }
        break;
      }
      default:
        err = "unknown constraint module";
        return -1;
    }
    if (!ok) { err = "too many inequality rows"; return -1; }
    M.mod_rows[mi] = row - M.mod_row0[mi];
  }
  M.nh = row; M.nfk = nfk;
  for (int j = 0; j < M.nv; j++)
    if (std::isfinite(d.lb[j])) { M.lb_var[M.nlb] = (int8_t)j; M.lb_val[M.nlb] = d.lb[j]; M.nlb++; }
  for (int j = 0; j < M.nv; j++)
    if (std::isfinite(d.ub[j])) { M.ub_var[M.nub] = (int8_t)j; M.ub_val[M.nub] = d.ub[j]; M.nub++; }
  M.m = M.nh + M.nlb + M.nub;
  M.max_iter = d.max_iter > 0 ? d.max_iter : 200;
  M.tol_stat = d.tol_stat > 0 ? d.tol_stat : 1e-6;
  M.tol_eq = d.tol_eq > 0 ? d.tol_eq : 1e-8;
  M.tol_ineq = d.tol_ineq > 0 ? d.tol_ineq : 1e-8;
  M.tol_comp = d.tol_comp > 0 ? d.tol_comp : 1e-6;
  M.mu0 = d.mu0 > 0 ? d.mu0 : 1.0;
  M.acc_iters = d.acc_iters < 0 ? 0 : d.acc_iters;
  M.acc_obj_tol = d.acc_obj_tol > 0 ? d.acc_obj_tol : 1e-8;
  M.ls_max = d.ls_max > 0 ? d.ls_max : kDescLsMax;
  // exact curvature of the distance rows: holonomic chain, no slack, and for n <= 3 every frame a
  // distance row refers to moves affinely with q (prismatic joints, or revolute at the frame itself) -- and the
  // goal's frame too when the model has a goal cost: its kinematic term exists only under Cfg::FKCURV (n > 3), so
  // with a goal on a frame that turns the terms would be those of a hybrid matrix, not of the exact Hessian
  auto affine = [&](int f) {
    for (int j = 0; j <= f; j++)
      if (d.joint_type[j] == RMPC_JOINT_REVOLUTE && j != f) return false;
    return true;
  };
  bool curv = d.robot == RMPC_ROBOT_CHAIN && d.ns == 0;
  // (the arms carry the kinematics' own second derivatives: Cfg::FKCURV)
  // (by row: the sphere and pair rows of the built-in modules and of the row-described ones alike)
  for (int r = 0; r < M.nh && curv && d.n <= 3; r++) {
    if (M.row_kind[r] == ROW_RADIAL) curv = curv && affine(M.row_a[r]);
    if (M.row_kind[r] == ROW_SELF) curv = curv && affine(M.row_a[r]) && affine(M.row_b[r]);
  }
  if (curv && d.n <= 3 && d.has_goal) curv = affine(d.end_frame);
  if (d.robot == RMPC_ROBOT_DIFFDRIVE) curv = true;   // exact second-order terms of the unicycle (Cfg::DDCURV)
  M.use_curv = curv ? 1 : 0;
  return 0;
}

// ---- generated views (rmpc_spec_gen.hpp) --------------------------------------------------
// Source text of the view of one descriptor: the accessors of RtView as constexpr functions over literal tables
// (doubles as hex floats: exact).  scripts/gen_specs.py writes rmpc_spec_gen.hpp from it for the shipped
// configurations; the library is then built with those views next to the runtime one.
static std::string spec_source(const rmpc_desc &d, const DevModel &M, const DevTables &T, const std::string &name) {
  std::string o;
  char buf[128];
  auto fi = [&](int v) { snprintf(buf, sizeof buf, "%d", v); return std::string(buf); };
  auto fd = [&](double v) { snprintf(buf, sizeof buf, "%a", v); return std::string(buf); };
  auto scalar = [&](const char *nm, int v) {
    o += "  __host__ __device__ static constexpr int " + std::string(nm) + "() { return " + fi(v) + "; }\n";
  };
  auto arr1 = [&](const char *nm, const int *p, int n) {
    o += "  __host__ __device__ static constexpr int " + std::string(nm) + "(int i) { constexpr int t[" + fi(n) + "] = {";
    for (int i = 0; i < n; i++) o += (i ? ", " : "") + fi(p[i]);
    o += "}; return t[i]; }\n";
  };
  auto arr2i = [&](const char *nm, const int *p, int n0, int n1) {
    o += "  __host__ __device__ static constexpr int " + std::string(nm) + "(int i, int j) { constexpr int t[" + fi(n0) + "][" + fi(n1) + "] = {";
    for (int i = 0; i < n0; i++) {
      o += (i ? ", {" : "{");
      for (int j = 0; j < n1; j++) o += (j ? ", " : "") + fi(p[i * n1 + j]);
      o += "}";
    }
    o += "}; return t[i][j]; }\n";
  };
  auto arr2d = [&](const char *nm, const double *p, int n0, int n1) {
    o += "  __host__ __device__ static constexpr double " + std::string(nm) + "(int i, int j) { constexpr double t[" + fi(n0) + "][" + fi(n1) + "] = {";
    for (int i = 0; i < n0; i++) {
      o += (i ? ", {" : "{");
      for (int j = 0; j < n1; j++) o += (j ? ", " : "") + fd(p[i * n1 + j]);
      o += "}";
    }
    o += "}; return t[i][j]; }\n";
  };
  o += "struct " + name + " {\n  static constexpr bool SPEC = true;\n";
  o += "  static constexpr int ROBOT = " + fi(d.robot) + ", NQ = " + fi(d.n) + ", NS = " + fi(d.ns) + ";\n";
  o += "  __host__ __device__ " + name + "() {}\n  __host__ __device__ " + name + "(const DevModel &, const DevTables &) {}\n";
  scalar("nslots", T.nslots);
  arr1("slot_fa", T.slot_fa, kMaxSlots);
  arr1("slot_fb", T.slot_fb, kMaxSlots);
  arr1("slot_row_begin", T.slot_row_begin, kMaxSlots + 1);
  scalar("nfkrows", T.nfkrows);
  arr1("fk_row", T.fk_row, kMaxFkRows);
  arr1("fk_kind", T.fk_kind, kMaxFkRows);
  arr1("fk_obst", T.fk_obst, kMaxFkRows);
  arr1("fk_mod", T.fk_mod, kMaxFkRows);
  arr1("fk_first", T.fk_first, kMaxFkRows);
  arr1("fk_idx", T.fk_idx, kMaxFkRows);
  arr2i("v_row", &T.v_row[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_sgn", &T.v_sgn[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_poff", &T.v_poff[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_soft", &T.v_soft[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_mod", &T.v_mod[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_first", &T.v_first[0][0], RMPC_NV_MAX, kVarRows);
  arr2d("v_val", &T.v_val[0][0], RMPC_NV_MAX, kVarRows);
  scalar("off_r_body", M.off_r_body); scalar("off_obst", M.off_obst); scalar("off_lin", M.off_lin);
  scalar("off_wu", M.off_wu); scalar("off_goal", M.off_goal); scalar("off_wgoal", M.off_wgoal);
  scalar("off_wconstr", M.off_wconstr); scalar("off_ws", M.off_ws);
  scalar("has_goal", M.has_goal); scalar("has_avoid", M.has_avoid);
  arr1("joint_type", M.joint_type, RMPC_MAX_JOINTS);
  arr2d("joint_xyz", &M.joint_xyz[0][0], RMPC_MAX_JOINTS, 3);
  arr2d("joint_rot", &M.joint_rot[0][0], RMPC_MAX_JOINTS, 9);
  arr2d("joint_axis", &M.joint_axis[0][0], RMPC_MAX_JOINTS, 3);
  arr2d("dd_off", &M.dd_off[0][0], RMPC_MAX_JOINTS, 3);
  o += "};\n";
  return o;
}

}  // namespace rmpc
