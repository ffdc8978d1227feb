// grx_host_tables.h -- everything that turns a grx_config into the CONTENTS of a handle's device tables, as plain host functions: they take
// the config and fill host structs / vectors, nothing else.  Included by grx_capi.cpp only, ahead of the definition of the handle, so that no
// builder can reach one or call the HIP runtime: grx_create (grx_capi.cpp) allocates, uploads and owns; a builder can be run without a device
// (grx_debug_trimesh_tables does).  Errors go through fail() (grx_capi.cpp), with the codes of include/grx.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/grx.h"
#include "grx_device.h"
#include "grx_rng.h"

namespace {

// the fused kernel is specialised for the GR1 lower-limb tree: base + two 5-joint chains with
// axes x, z, y, y, y and unrotated joint frames (GR1T1_lower_limb.urdf / GR1T2_lower_limb.urdf)
int check_topology(const grx_model& m) {
    if (m.num_bodies != 1 + GRX_ND) return fail(GRX_ERR_UNSUPPORTED_MODEL, "HIP path supports 10-DOF lower-limb models (2 chains x 5 joints); got num_bodies=" + std::to_string(m.num_bodies));
    static const int axes[GRX_LEG] = {0, 2, 1, 1, 1};
    for (int side = 0; side < 2; ++side)
        for (int k = 0; k < GRX_LEG; ++k) {
            int b = 1 + side * GRX_LEG + k;
            int want_parent = k == 0 ? 0 : b - 1;
            if (m.parent[b] != want_parent) return fail(GRX_ERR_UNSUPPORTED_MODEL, "unsupported tree: body " + std::to_string(b) + " parent " + std::to_string(m.parent[b]));
            for (int a = 0; a < 3; ++a) {
                float want = a == axes[k] ? 1.f : 0.f;
                if (fabsf(m.joint_axis[b][a] - want) > 1e-6f) return fail(GRX_ERR_UNSUPPORTED_MODEL, "unsupported joint axis on body " + std::to_string(b));
            }
            static const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            for (int a = 0; a < 9; ++a)
                if (fabsf(m.joint_rot0[b][a] - I9[a]) > 1e-6f) return fail(GRX_ERR_UNSUPPORTED_MODEL, "rotated joint frame on body " + std::to_string(b));
        }
    for (int f = 0; f < 2; ++f)
        if (m.foot_body[f] != (f + 1) * GRX_LEG) return fail(GRX_ERR_UNSUPPORTED_MODEL, "feet must be the chain leaves");
    if (m.torso_body > 0 || m.forehead_body > 0) return fail(GRX_ERR_UNSUPPORTED_MODEL, "torso/forehead must ride on the base lump");
    return GRX_OK;
}

int build_side_tables(const grx_config& c, KTables& P, uint32_t* ll_mask, uint64_t* sp_mask) {
    const grx_model& m = c.model;
    memset(P.side, 0, sizeof P.side);
    *ll_mask = 0;
    *sp_mask = 0;
    for (int side = 0; side < 2; ++side) {
        SideConst& S = P.side[side];
        for (int k = 0; k < GRX_LEG; ++k) {
            int b = 1 + side * GRX_LEG + k, j = b - 1;
            for (int a = 0; a < 3; ++a) { S.body[k].r[a] = m.joint_pos[b][a]; S.body[k].com[a] = m.com[b][a]; }
            for (int a = 0; a < 6; ++a) S.body[k].Ic[a] = m.inertia[b][a];
            S.body[k].mass = m.mass[b];
            S.body[k].kp = c.kp[j]; S.body[k].kd = c.kd[j]; S.body[k].q0 = c.default_dof_pos[j];
            S.body[k].effort = m.dof_effort[j]; S.body[k].vlim = m.dof_vel_limit[j];
            S.body[k].qlo = m.dof_lower[j]; S.body[k].qhi = m.dof_upper[j];
            S.body[k].Klim = c.contact.k_limit * m.dof_effort[j];
            S.body[k].Clim = c.contact.c_limit * S.body[k].Klim;
            S.body[k].amin = c.clip_actions_min[j]; S.body[k].amax = c.clip_actions_max[j];
            float mid = (m.dof_lower[j] + m.dof_upper[j]) / 2, rng = m.dof_upper[j] - m.dof_lower[j];
            S.body[k].slo = mid - 0.5f * rng * c.soft_dof_pos_limit;
            S.body[k].shi = mid + 0.5f * rng * c.soft_dof_pos_limit;
        }
        for (int a = 0; a < 3; ++a) S.foot_pos[a] = m.foot_pos[side][a];
    }
    // spheres: chain spheres go to their side; base-lump spheres are split between the two lanes
    // at a LINK boundary (per-link force netting must see a whole link on one lane)
    std::vector<int> base_idx;
    for (int i = 0; i < m.num_spheres; ++i) {
        int b = m.sph_body[i];
        if (b < 0 || b >= m.num_bodies) return fail(GRX_ERR_INVALID_ARGUMENT, "sphere body out of range");
        if (m.sph_link[i] < 0 || m.sph_link[i] >= GRX_MAX_LINKS) return fail(GRX_ERR_INVALID_ARGUMENT, "sph_link out of range");
        if (b == 0) base_idx.push_back(i);
        else if (m.sph_flags[i] & (GRX_SPH_TERMINATE | GRX_SPH_PENALISE))
            return fail(GRX_ERR_UNSUPPORTED_MODEL, "terminating/penalised shapes must ride on the base lump");
    }
    // base_idx is sorted by link (model.py emits spheres sorted by (body, link)); cut near the middle
    size_t cut = base_idx.size() / 2;
    while (cut > 0 && cut < base_idx.size() && m.sph_link[base_idx[cut]] == m.sph_link[base_idx[cut - 1]]) ++cut;
    // fixed table layout per lane: [0..7] base-lump share, [8,9] chain body 2 (thigh_pitch), [10,11] body 3 (shank),
    // [12..15] body 4 (foot, anchored).  Unused slots are parked far above any terrain (r = -1e30).
    static const int cnt[GRX_LEG] = {0, 0, 2, 2, 4}, off[GRX_LEG] = {8, 8, 8, 10, 12};
    auto put = [&](SphC& o, int i, int slot) {
        o.x = m.sph_pos[i][0]; o.y = m.sph_pos[i][1]; o.z = m.sph_pos[i][2]; o.r = m.sph_radius[i];
        o.flags = m.sph_flags[i]; o.slot = slot; o.link_last = (m.sph_link[i] + 1) << 8; o.dmax = m.sph_damp_max[i];
    };
    for (int side = 0; side < 2; ++side) {
        SideConst& S = P.side[side];
        for (int i = 0; i < GRX_MAXSPH_SIDE; ++i) { S.sph[i] = SphC{0.f, 0.f, 0.f, -1e30f, 0u, -1, 0, 0.f}; }
        size_t lo = side == 0 ? 0 : cut, hi = side == 0 ? cut : base_idx.size();
        if (hi - lo > 8) return fail(GRX_ERR_UNSUPPORTED_MODEL, "more than 8 base-lump collision spheres per lane");
        for (size_t n = lo; n < hi; ++n) {
            SphC& o = S.sph[n - lo];
            put(o, base_idx[n], -1);
            bool last = (n + 1 == hi) || m.sph_link[base_idx[n + 1]] != m.sph_link[base_idx[n]];
            o.link_last |= last ? 1 : 0;
        }
        for (int k = 0; k < GRX_LEG; ++k) {
            int b = 1 + side * GRX_LEG + k, n = 0;
            for (int i = 0; i < m.num_spheres; ++i) {
                if (m.sph_body[i] != b) continue;
                bool foot = m.sph_flags[i] & (side == 0 ? GRX_SPH_FOOT_LEFT : GRX_SPH_FOOT_RIGHT);
                if (m.sph_flags[i] & (side == 0 ? GRX_SPH_FOOT_RIGHT : GRX_SPH_FOOT_LEFT))
                    return fail(GRX_ERR_UNSUPPORTED_MODEL, "foot shape on the wrong chain");
                if (n >= cnt[k]) return fail(GRX_ERR_UNSUPPORTED_MODEL, "collision shapes on chain body " + std::to_string(k) + " exceed the kernel's table (0,0,2,2,4)");
                if (foot != (k == GRX_LEG - 1)) return fail(GRX_ERR_UNSUPPORTED_MODEL, "anchored foot shapes must sit on the chain leaf");
                put(S.sph[off[k] + n], i, foot ? n : -1);
                if (n > 0 && m.sph_link[i] != sph_link(S.sph[off[k]]))   // GRX_T_CONTACT_FORCES nets a chain body's shapes into one row
                    return fail(GRX_ERR_UNSUPPORTED_MODEL, "the collision shapes of a chain body must belong to one URDF link");
                ++n;
            }
        }
        // bounding sphere of the shapes of chain bodies 2, 3, 4 (body frame): broad phase of the leg-vs-leg self-collision
        for (int bi = 0; bi < 3; ++bi) {
            const int k = 2 + bi;
            float cx = 0, cy = 0, cz = 0;
            for (int n = 0; n < cnt[k]; ++n) { const SphC& q = S.sph[off[k] + n]; cx += q.x; cy += q.y; cz += q.z; }
            cx /= cnt[k]; cy /= cnt[k]; cz /= cnt[k];
            float rad = 0;
            for (int n = 0; n < cnt[k]; ++n) {
                const SphC& q = S.sph[off[k] + n];
                if (q.r < 0) continue;
                rad = std::max(rad, sqrtf((q.x - cx) * (q.x - cx) + (q.y - cy) * (q.y - cy) + (q.z - cz) * (q.z - cz)) + q.r);
            }
            S.bs[bi][0] = cx; S.bs[bi][1] = cy; S.bs[bi][2] = cz; S.bs[bi][3] = rad;
        }
    }
    // self-collision pairs (grx_model.pair_a / pair_b) -> the fused kernel's tables: left-leg x right-leg body pairs
    // (every sphere pair of a listed link pair is in the list, so a 3 x 3 body mask carries it) and base-lump x thigh pairs
    for (int pi = 0; pi < m.num_pairs; ++pi) {
        int ia = m.pair_a[pi], ib = m.pair_b[pi];
        if (ia < 0 || ib < 0 || ia >= m.num_spheres || ib >= m.num_spheres) return fail(GRX_ERR_INVALID_ARGUMENT, "self-collision pair out of range");
        int ba = m.sph_body[ia], bb = m.sph_body[ib];
        if (ba > bb) { std::swap(ia, ib); std::swap(ba, bb); }
        if (ba == 0 && bb == 0) continue;
        auto side_of = [](int b) { return (b - 1) / GRX_LEG; };
        auto k_of = [](int b) { return (b - 1) % GRX_LEG; };
        if (ba == 0) {   // base lump x chain shape: thigh shapes only
            const int side = side_of(bb), k = k_of(bb);
            if (k != 2) return fail(GRX_ERR_UNSUPPORTED_MODEL, "base-lump self-collision with a chain body other than the thigh");
            SideConst& S = P.side[side];
            int tsel = -1;
            for (int n = 0; n < cnt[2]; ++n) {
                const SphC& q = S.sph[off[2] + n];
                if (q.x == m.sph_pos[ib][0] && q.y == m.sph_pos[ib][1] && q.z == m.sph_pos[ib][2]) tsel = n;
            }
            if (tsel < 0 || tsel > 1) return fail(GRX_ERR_UNSUPPORTED_MODEL, "base-lump / thigh self-collision: unknown thigh shape");
            int at = -1;   // one entry per base-lump sphere (entries of one link stay adjacent: the pairs arrive sorted by sphere)
            for (int n = 0; n < S.nbc; ++n)
                if (S.bc[n].x == m.sph_pos[ia][0] && S.bc[n].y == m.sph_pos[ia][1] && S.bc[n].z == m.sph_pos[ia][2] && S.bc[n].link == m.sph_link[ia] &&
                    S.bc[n].r == m.sph_radius[ia] && S.bc[n].dmax == m.sph_damp_max[ia]) at = n;   // (coincident spheres of different size or damping stay apart)
            if (at < 0) {
                if (S.nbc >= GRX_MAX_BC) return fail(GRX_ERR_UNSUPPORTED_MODEL, "base-lump / thigh self-collision table overflow");
                at = S.nbc++;
                BaseChainPair& e = S.bc[at];
                e.x = m.sph_pos[ia][0]; e.y = m.sph_pos[ia][1]; e.z = m.sph_pos[ia][2]; e.r = m.sph_radius[ia];
                e.dmax = m.sph_damp_max[ia]; e.tmask = 0; e.link = m.sph_link[ia]; e.pad = 0;
            }
            S.bc[at].tmask |= 1 << tsel;
        } else {
            if (side_of(ba) == side_of(bb)) return fail(GRX_ERR_UNSUPPORTED_MODEL, "self-collision within one leg chain");
            const int kl = side_of(ba) == 0 ? k_of(ba) : k_of(bb), kr = side_of(ba) == 0 ? k_of(bb) : k_of(ba);
            if (kl < 2 || kr < 2) return fail(GRX_ERR_UNSUPPORTED_MODEL, "self-collision shapes on a chain body without a shape table");
            *ll_mask |= 1u << ((kl - 2) * 3 + (kr - 2));
            // the sphere pair itself: table slots of the left-lane and the right-lane shape
            const int il = side_of(ba) == 0 ? ia : ib, ir = side_of(ba) == 0 ? ib : ia;
            auto slot_of = [&](int side, int k, int isph) {
                const SideConst& S = P.side[side];
                for (int n = 0; n < cnt[k]; ++n) {
                    const SphC& q = S.sph[off[k] + n];
                    if (q.x == m.sph_pos[isph][0] && q.y == m.sph_pos[isph][1] && q.z == m.sph_pos[isph][2]) return off[k] + n;
                }
                return -1;
            };
            const int sl = slot_of(0, kl, il), sr = slot_of(1, kr, ir);
            if (sl < 0 || sr < 0) return fail(GRX_ERR_UNSUPPORTED_MODEL, "leg x leg self-collision shape not in the kernel's tables");
            *sp_mask |= 1ull << ((sl - 8) * 8 + (sr - 8));
        }
    }
    return GRX_OK;
}

// GRX_T_RIGID_BODY_STATES tables of the fused kernel: chain links go to their leg's lane, the base lump's links alternate
void rot_to_quat(const float R[9], float q[4]) {   // row-major rotation -> xyzw, largest-component form
    const float t0 = 1 + R[0] - R[4] - R[8], t1 = 1 - R[0] + R[4] - R[8], t2 = 1 - R[0] - R[4] + R[8], t3 = 1 + R[0] + R[4] + R[8];
    if (t3 >= t0 && t3 >= t1 && t3 >= t2) { q[0] = R[7] - R[5]; q[1] = R[2] - R[6]; q[2] = R[3] - R[1]; q[3] = t3; }
    else if (t0 >= t1 && t0 >= t2) { q[0] = t0; q[1] = R[1] + R[3]; q[2] = R[2] + R[6]; q[3] = R[7] - R[5]; }
    else if (t1 >= t2) { q[0] = R[1] + R[3]; q[1] = t1; q[2] = R[5] + R[7]; q[3] = R[2] - R[6]; }
    else { q[0] = R[2] + R[6]; q[1] = R[5] + R[7]; q[2] = t2; q[3] = R[3] - R[1]; }
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
}
int build_rbs_tables(const grx_model& m, RbsTables& T) {
    memset(&T, 0, sizeof T);
    if (m.num_links < 0 || m.num_links > GRX_MAX_LINKS) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_model.num_links out of range");
    int nbase = 0;
    std::vector<int> lists[2][GRX_LEG + 1];
    for (int l = 0; l < m.num_links; ++l) {
        const int b = m.link_body[l];
        if (b < 0 || b >= m.num_bodies) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_model.link_body out of range");
        if (b == 0) lists[(nbase++) & 1][0].push_back(l);
        else lists[(b - 1) / GRX_LEG][1 + (b - 1) % GRX_LEG].push_back(l);
    }
    for (int side = 0; side < 2; ++side) {
        int n = 0;
        for (int lvl = 0; lvl <= GRX_LEG; ++lvl) {
            T.off[side][lvl] = n;
            for (int l : lists[side][lvl]) {
                if (n >= GRX_RBS_MAX) return fail(GRX_ERR_UNSUPPORTED_MODEL, "more link frames per lane than the rigid-body-state table holds");
                RbsEntry& E = T.e[side][n++];
                E.px = m.link_pos[l][0]; E.py = m.link_pos[l][1]; E.pz = m.link_pos[l][2]; E.link = l;
                float q[4];
                rot_to_quat(m.link_rot[l], q);
                E.qx = q[0]; E.qy = q[1]; E.qz = q[2]; E.qw = q[3];
            }
        }
        T.off[side][GRX_LEG + 1] = n;
    }
    return GRX_OK;
}

/* c10::div_floor_floating (what torch.div(..., rounding_mode='floor') evaluates in float32) */
float torch_div_floor(float a, float b) {
    float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.0f && ((b < 0.0f) != (mod < 0.0f))) div -= 1.0f;
    if (div == 0.0f) return copysignf(0.0f, a / b);
    float fl = floorf(div);
    if (div - fl > 0.5f) fl += 1.0f;
    return fl;
}

// randomised base lump (oracle base_lump(); legged_robot.py:618-648)
void base_lump(const grx_model& m, float link_mass, const float link_com[3], float* M_out, float c_out[3], float I_out[6]) {
    float m1 = m.base_rest_mass, m2 = link_mass;
    float scale = m.base_link_mass > 0 ? m2 / m.base_link_mass : 1.f;
    float M = m1 + m2, c[3], I[6];
    for (int i = 0; i < 3; ++i) c[i] = (m1 * m.base_rest_com[i] + m2 * link_com[i]) / M;
    for (int i = 0; i < 6; ++i) I[i] = m.base_rest_inertia[i] + scale * m.base_link_inertia[i];
    const float* cs[2] = {m.base_rest_com, link_com};
    float ms[2] = {m1, m2};
    for (int k = 0; k < 2; ++k) {
        float d[3] = {cs[k][0] - c[0], cs[k][1] - c[1], cs[k][2] - c[2]};
        float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        I[0] += ms[k] * (dd - d[0] * d[0]); I[1] -= ms[k] * d[0] * d[1]; I[2] -= ms[k] * d[0] * d[2];
        I[3] += ms[k] * (dd - d[1] * d[1]); I[4] -= ms[k] * d[1] * d[2];
        I[5] += ms[k] * (dd - d[2] * d[2]);
    }
    *M_out = M;
    for (int i = 0; i < 3; ++i) c_out[i] = c[i];
    for (int i = 0; i < 6; ++i) I_out[i] = I[i];
}

// ---- mesh_type 'trimesh': the reference's slope-corrected triangle mesh as per-cell tables
// legged_robot.py:903-921 hands PhysX convert_heightfield_to_trimesh(raster, slope_threshold) (isaacgym terrain_utils.py:286-350): the raster's
// heights on vertices that were MOVED by whole cells -- a vertex whose +x / -x / +y / -y (or, where those do not move it, diagonal) neighbour
// stands more than the threshold above it goes under that neighbour (:313-325), which turns the steep cell into a vertical face.  All vertices
// stay on grid points, so the mesh above one raster cell is: a plane per triangle half of the cell (the halves of :335-347; at a concave corner
// the two halves can sit on different levels) and vertical faces on grid lines.  Tables (grx_device.h KParams::tm_off, read by terrain_eval /
// wall_contact in grx_kernels.hip; the oracle builds its own in trimesh_build):
//   ground[cell][6]: corner heights of the top surface under half 0 (ty >= tx: e00, e01, e11) and half 1 (tx > ty: e00, e10, e11) -- the plane
//     a vertical ray hits at the half's centroid, evaluated at the cell's corners, in raster units (rounded: a sloped neighbour stretched over
//     two cells leaves half units);
//   walls[cell][8]: tops of the vertical faces on the sides x-, x+, y-, y+ (the rectangle both of whose ends the faces reach) and of the posts at
//     the corners 00, 10, 01, 11 (the end of a face that runs away from the corner), where they rise above the cell's own ground; else TM_NONE.
constexpr int16_t TM_NONE = INT16_MIN;
struct TrimeshTables { std::vector<int16_t> ground, walls; };
struct TmVertex { double x, y, z; };
TrimeshTables build_trimesh_tables(const grx_config& c) {
    const int R = c.hf_rows, C = c.hf_cols;
    const int16_t* H = c.height_samples;
    const size_t n = (size_t)R * C;
    const double thr = (double)c.slope_threshold * ((double)c.horizontal_scale / (double)c.vertical_scale);   // raster units, in double like numpy (:310)
    auto at = [&](int i, int j) { return (int)H[(size_t)i * C + j]; };
    auto above = [&](int i, int j, int di, int dj) {   // the neighbour stands more than the threshold above (i, j)
        const int a = i + di, b = j + dj;
        return a >= 0 && a < R && b >= 0 && b < C && at(a, b) - at(i, j) > thr ? 1 : 0;
    };
    std::vector<int8_t> mx(n), my(n);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < C; ++j) {
            const int sx = above(i, j, 1, 0) - above(i, j, -1, 0), sy = above(i, j, 0, 1) - above(i, j, 0, -1), sc = above(i, j, 1, 1) - above(i, j, -1, -1);
            mx[(size_t)i * C + j] = (int8_t)(sx != 0 ? sx : sc);   // xx += move_x + move_corners * (move_x == 0)   (:324)
            my[(size_t)i * C + j] = (int8_t)(sy != 0 ? sy : sc);
        }
    auto vertex = [&](int i, int j) { const size_t k = (size_t)i * C + j; return TmVertex{(double)(i + mx[k]), (double)(j + my[k]), (double)H[k]}; };
    auto triangle = [&](int a, int b, int second, TmVertex t[3]) {   // (ind0, ind3, ind1) and (ind0, ind2, ind3) of :339-347
        t[0] = vertex(a, b);
        t[1] = second ? vertex(a + 1, b) : vertex(a + 1, b + 1);
        t[2] = second ? vertex(a + 1, b + 1) : vertex(a, b + 1);
    };
    auto round16 = [](double z) { return (int16_t)lrint(std::min(std::max(z, -32767.0), 32767.0)); };
    // the plane of the highest triangle over the raster point (px, py): z there and its gradient
    auto plane_at = [&](double px, double py, double pl[3]) {
        const int ci = (int)floor(px), cj = (int)floor(py);
        bool found = false;
        for (int a = std::max(ci - 1, 0); a <= std::min(ci + 1, R - 2); ++a)
            for (int b = std::max(cj - 1, 0); b <= std::min(cj + 1, C - 2); ++b)
                for (int k = 0; k < 2; ++k) {
                    TmVertex t[3];
                    triangle(a, b, k, t);
                    const double ux = t[1].x - t[0].x, uy = t[1].y - t[0].y, vx = t[2].x - t[0].x, vy = t[2].y - t[0].y;
                    const double den = ux * vy - vx * uy;
                    if (fabs(den) < 1e-9) continue;   // projects to a segment: a vertical face
                    const double qx = px - t[0].x, qy = py - t[0].y;
                    const double w1 = (qx * vy - vx * qy) / den, w2 = (ux * qy - qx * uy) / den;
                    if (w1 < -1e-9 || w2 < -1e-9 || 1 - w1 - w2 < -1e-9) continue;
                    const double uz = t[1].z - t[0].z, vz = t[2].z - t[0].z, z = t[0].z + w1 * uz + w2 * vz;
                    if (!found || z > pl[0]) { pl[0] = z; pl[1] = (uz * vy - vz * uy) / den; pl[2] = (ux * vz - vx * uz) / den; found = true; }
                }
        return found;
    };
    TrimeshTables out;
    out.ground.resize(6 * n);
    out.walls.assign(8 * n, TM_NONE);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < C; ++j) {
            const int i1 = std::min(i + 1, R - 1), j1 = std::min(j + 1, C - 1);
            int16_t* e = &out.ground[6 * ((size_t)i * C + j)];
            e[0] = e[3] = (int16_t)at(i, j); e[1] = (int16_t)at(i, j1); e[4] = (int16_t)at(i1, j); e[2] = e[5] = (int16_t)at(i1, j1);
            if (i > R - 2 || j > C - 2) continue;
            bool touched = false;   // only a moved vertex within the 3 x 3 cells around this one can change what lies over it
            for (int a = std::max(i - 1, 0); a <= std::min(i + 2, R - 1) && !touched; ++a)
                for (int b = std::max(j - 1, 0); b <= std::min(j + 2, C - 1) && !touched; ++b) touched = mx[(size_t)a * C + b] != 0 || my[(size_t)a * C + b] != 0;
            if (!touched) continue;
            for (int half = 0; half < 2; ++half) {
                const double px = i + (half ? 2.0 : 1.0) / 3, py = j + (half ? 1.0 : 2.0) / 3;   // the half's centroid
                double pl[3];
                if (!plane_at(px, py, pl)) continue;
                auto corner = [&](int ci, int cj) { return round16(pl[0] + pl[1] * (ci - px) + pl[2] * (cj - py)); };
                e[3 * half] = corner(i, j);
                e[3 * half + 1] = half ? corner(i + 1, j) : corner(i, j + 1);
                e[3 * half + 2] = corner(i + 1, j + 1);
            }
        }
    // the vertical faces, per unit segment of a grid line and per END of the segment: line x = X, y in [k, k + 1] -> fx[2 * (X * C + k) + end];
    // line y = Y, x in [k, k + 1] -> fy[2 * (Y * R + k) + end].  (Where three levels meet, the vertices slid along a face leave it triangular.)
    std::vector<int16_t> fx(2 * n, TM_NONE), fy(2 * n, TM_NONE);
    for (int a = 0; a < R - 1; ++a)
        for (int b = 0; b < C - 1; ++b)
            for (int k = 0; k < 2; ++k) {
                TmVertex t[3];
                triangle(a, b, k, t);
                if (fabs((t[1].x - t[0].x) * (t[2].y - t[0].y) - (t[2].x - t[0].x) * (t[1].y - t[0].y)) > 1e-9) continue;
                if (std::max({t[0].z, t[1].z, t[2].z}) <= std::min({t[0].z, t[1].z, t[2].z})) continue;
                const bool on_x_line = t[0].x == t[1].x && t[0].x == t[2].x, on_y_line = t[0].y == t[1].y && t[0].y == t[2].y;
                if (on_x_line == on_y_line) continue;   // a needle, or a face across the grid (axis-aligned steps make none)
                double pos[3];
                for (int q = 0; q < 3; ++q) pos[q] = on_x_line ? t[q].y : t[q].x;
                const int line = (int)(on_x_line ? t[0].x : t[0].y), lo = (int)std::min({pos[0], pos[1], pos[2]}), hi = (int)std::max({pos[0], pos[1], pos[2]});
                const int nlines = on_x_line ? R : C, nseg = on_x_line ? C - 1 : R - 1, stride = on_x_line ? C : R;
                if (line < 0 || line >= nlines) continue;
                std::vector<int16_t>& f = on_x_line ? fx : fy;
                for (int q = std::max(lo, 0); q < std::min(hi, nseg); ++q)
                    for (int end = 0; end < 2; ++end) {
                        const double where = q + end;
                        double top = -1e30;   // the triangle's highest point over `where`
                        for (int m0 = 0; m0 < 3; ++m0) {
                            const int m1 = (m0 + 1) % 3;
                            if (where < std::min(pos[m0], pos[m1]) || where > std::max(pos[m0], pos[m1])) continue;
                            top = std::max(top, pos[m0] == pos[m1] ? std::max(t[m0].z, t[m1].z) : t[m0].z + (t[m1].z - t[m0].z) * (where - pos[m0]) / (pos[m1] - pos[m0]));
                        }
                        int16_t& o = f[2 * ((size_t)line * stride + q) + end];
                        if (top > -1e29) o = std::max(o, round16(top));
                    }
            }
    auto face_x = [&](int X, int k, int end) { return X >= 0 && X < R && k >= 0 && k < C - 1 ? fx[2 * ((size_t)X * C + k) + end] : TM_NONE; };
    auto face_y = [&](int Y, int k, int end) { return Y >= 0 && Y < C && k >= 0 && k < R - 1 ? fy[2 * ((size_t)Y * R + k) + end] : TM_NONE; };
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < C; ++j) {
            const int16_t* e = &out.ground[6 * ((size_t)i * C + j)];
            int16_t* w = &out.walls[8 * ((size_t)i * C + j)];
            const int16_t side[4] = {std::min(face_x(i, j, 0), face_x(i, j, 1)), std::min(face_x(i + 1, j, 0), face_x(i + 1, j, 1)),
                                     std::min(face_y(j, i, 0), face_y(j, i, 1)), std::min(face_y(j + 1, i, 0), face_y(j + 1, i, 1))};
            // the cell's own ground along the side (x- and y+ bound half 0, x+ and y- half 1)
            const int16_t ground[4] = {std::max(e[0], e[1]), std::max(e[4], e[5]), std::max(e[3], e[4]), std::max(e[1], e[2])};
            for (int q = 0; q < 4; ++q) w[q] = side[q] > ground[q] ? side[q] : TM_NONE;
            const int16_t away_x[4] = {face_x(i, j - 1, 1), face_x(i + 1, j - 1, 1), face_x(i, j + 1, 0), face_x(i + 1, j + 1, 0)};
            const int16_t away_y[4] = {face_y(j, i - 1, 1), face_y(j, i + 1, 0), face_y(j + 1, i - 1, 1), face_y(j + 1, i + 1, 0)};
            const int16_t corner[4] = {std::max(e[0], e[3]), e[4], e[1], std::max(e[2], e[5])};   // 00, 10, 01, 11
            for (int q = 0; q < 4; ++q) { const int16_t top = std::max(away_x[q], away_y[q]); w[4 + q] = top > corner[q] ? top : TM_NONE; }
        }
    return out;
}

// ---- generic-tree path: grx_generic.h's GenTables -- the struct text the kernels compile, in this translation unit's own anonymous namespace
#include "grx_gen_tables.h"

// GenTables of a model (the one-lane generic kernel's tables, and what the tree kernel's are derived from); pos_of: model sphere index -> position
// in the tables, whose spheres are sorted by carrying body
int build_gen_tables(const grx_config& c, GenTables& T, std::vector<int>& pos_of) {
    const grx_model& m = c.model;
    if (m.num_spheres > GRX_MAX_SPHERES) return fail(GRX_ERR_UNSUPPORTED_MODEL, "too many collision spheres");
    memset(&T, 0, sizeof T);
    T.nb = m.num_bodies; T.nd = m.num_bodies - 1; T.nsph = m.num_spheres;
    for (int b = 0; b < m.num_bodies; ++b) {
        T.parent[b] = m.parent[b];
        if (b > 0 && (m.parent[b] < 0 || m.parent[b] >= b)) return fail(GRX_ERR_UNSUPPORTED_MODEL, "bodies must be listed parents first");
        for (int a = 0; a < 3; ++a) { T.axis[b][a] = m.joint_axis[b][a]; T.jpos[b][a] = m.joint_pos[b][a]; T.com[b][a] = m.com[b][a]; }
        for (int a = 0; a < 9; ++a) T.rot0[b][a] = m.joint_rot0[b][a];
        for (int a = 0; a < 6; ++a) T.Ic[b][a] = m.inertia[b][a];
        T.mass[b] = m.mass[b];
    }
    for (int j = 0; j < T.nd; ++j) {
        T.kp[j] = c.kp[j]; T.kd[j] = c.kd[j]; T.q0[j] = c.default_dof_pos[j];
        T.effort[j] = m.dof_effort[j]; T.vlim[j] = m.dof_vel_limit[j]; T.qlo[j] = m.dof_lower[j]; T.qhi[j] = m.dof_upper[j];
        T.Klim[j] = c.contact.k_limit * m.dof_effort[j];
        T.Clim[j] = c.contact.c_limit * T.Klim[j];
        T.arm[j] = m.dof_armature[j];
        T.amin[j] = c.clip_actions_min[j]; T.amax[j] = c.clip_actions_max[j];
        const float mid = (m.dof_lower[j] + m.dof_upper[j]) / 2, rng = m.dof_upper[j] - m.dof_lower[j];
        T.slo[j] = mid - 0.5f * rng * c.soft_dof_pos_limit;
        T.shi[j] = mid + 0.5f * rng * c.soft_dof_pos_limit;
    }
    // spheres sorted by carrying body (stable: model.py emits them sorted by (body, link) already)
    std::vector<int> order(m.num_spheres);
    for (int i = 0; i < m.num_spheres; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return m.sph_body[a] < m.sph_body[b]; });
    std::vector<int> link_ids;   // compact ids of the URDF links that carry shapes
    int foot_slots[2] = {0, 0};
    for (int f = 0; f < 2; ++f) T.foot_link[f] = -1;
    for (int k = 0; k < m.num_spheres; ++k) {
        const int i = order[k], b = m.sph_body[i];
        if (b < 0 || b >= m.num_bodies) return fail(GRX_ERR_INVALID_ARGUMENT, "sphere body out of range");
        T.sx[k] = m.sph_pos[i][0]; T.sy[k] = m.sph_pos[i][1]; T.sz[k] = m.sph_pos[i][2]; T.sr[k] = m.sph_radius[i]; T.sdmax[k] = m.sph_damp_max[i];
        int lc = -1;
        for (size_t t = 0; t < link_ids.size(); ++t) if (link_ids[t] == m.sph_link[i]) lc = (int)t;
        if (lc < 0) { lc = (int)link_ids.size(); link_ids.push_back(m.sph_link[i]); }
        if (lc >= GEN_MAXLC) return fail(GRX_ERR_UNSUPPORTED_MODEL, "too many links carry collision shapes");
        if (m.sph_link[i] < 0 || m.sph_link[i] >= GRX_MAX_LINKS) return fail(GRX_ERR_INVALID_ARGUMENT, "sph_link out of range");
        T.link_urdf[lc] = m.sph_link[i];
        T.slink[k] = lc;
        T.link_flags[lc] |= m.sph_flags[i] & (GRX_SPH_TERMINATE | GRX_SPH_PENALISE);
        T.sslot[k] = -1;
        for (int f = 0; f < 2; ++f)
            if (m.sph_flags[i] & (f == 0 ? GRX_SPH_FOOT_LEFT : GRX_SPH_FOOT_RIGHT)) {
                if (foot_slots[f] >= 4) return fail(GRX_ERR_UNSUPPORTED_MODEL, "more than 4 anchored spheres on a foot");
                T.sslot[k] = f * 4 + foot_slots[f]++;
                T.foot_link[f] = lc;
            }
    }
    T.nlc = (int)link_ids.size();
    {   // a compact link's shapes are contiguous (spheres sorted by (body, link)): ranges + bounding spheres (body frame)
        pos_of.assign(m.num_spheres, 0);   // model sphere index -> position in the sorted tables
        for (int k = 0; k < m.num_spheres; ++k) pos_of[order[k]] = k;
        for (int l = 0; l <= T.nlc; ++l) T.lc_begin[l] = m.num_spheres;
        for (int k = m.num_spheres - 1; k >= 0; --k) T.lc_begin[T.slink[k]] = k;
        for (int l = T.nlc - 1; l >= 0; --l) if (T.lc_begin[l] > T.lc_begin[l + 1]) return fail(GRX_ERR_UNSUPPORTED_MODEL, "collision shapes of a link are not contiguous");
        auto bound = [&](int l, float out4[4]) {
            float c[3] = {0, 0, 0};
            const int b0 = T.lc_begin[l], b1 = T.lc_begin[l + 1];
            for (int k = b0; k < b1; ++k) { c[0] += T.sx[k]; c[1] += T.sy[k]; c[2] += T.sz[k]; }
            for (int a = 0; a < 3; ++a) c[a] /= (float)(b1 - b0);
            float rad = 0;
            for (int k = b0; k < b1; ++k)
                rad = std::max(rad, sqrtf((T.sx[k] - c[0]) * (T.sx[k] - c[0]) + (T.sy[k] - c[1]) * (T.sy[k] - c[1]) + (T.sz[k] - c[2]) * (T.sz[k] - c[2])) + T.sr[k]);
            out4[0] = c[0]; out4[1] = c[1]; out4[2] = c[2]; out4[3] = rad;
        };
        T.nlp = 0;
        for (int pi = 0; pi < m.num_pairs; ++pi) {
            int ka = pos_of[m.pair_a[pi]], kb = pos_of[m.pair_b[pi]];
            int la = T.slink[ka], lb = T.slink[kb];
            int ba = m.sph_body[order[ka]], bb = m.sph_body[order[kb]];
            if (ba > bb) { std::swap(la, lb); std::swap(ba, bb); }   // body bb is never the base (workspace addressing)
            bool seen = false;
            for (int q = 0; q < T.nlp; ++q) seen = seen || (T.lp_a[q] == la && T.lp_b[q] == lb);
            if (seen) continue;
            if (ba == bb) return fail(GRX_ERR_INVALID_ARGUMENT, "self-collision pair within one body");
            if (T.nlp >= GEN_MAXLP) return fail(GRX_ERR_UNSUPPORTED_MODEL, "too many self-collision link pairs");
            T.lp_a[T.nlp] = la; T.lp_b[T.nlp] = lb; T.lp_ba[T.nlp] = ba; T.lp_bb[T.nlp] = bb;
            bound(la, T.lp_ca[T.nlp]); bound(lb, T.lp_cb[T.nlp]);
            ++T.nlp;
        }
    }
    for (int f = 0; f < 2; ++f) if (T.foot_link[f] < 0) return fail(GRX_ERR_UNSUPPORTED_MODEL, "a foot carries no collision shape");
    {
        int k = 0;
        for (int b = 0; b <= m.num_bodies; ++b) {
            while (k < m.num_spheres && m.sph_body[order[k]] < b) ++k;
            T.sph_begin[b] = k;
        }
    }
    for (int f = 0; f < 2; ++f) { T.foot_body[f] = m.foot_body[f]; for (int a = 0; a < 3; ++a) T.foot_pos[f][a] = m.foot_pos[f][a]; }
    T.torso_body = m.torso_body; T.forehead_body = m.forehead_body;
    memcpy(T.torso_rot, m.torso_rot, sizeof T.torso_rot);
    memcpy(T.forehead_rot, m.forehead_rot, sizeof T.forehead_rot);
    return GRX_OK;
}

// The lane-group tree kernel's table (grx_tree.h) for G lanes per env: chains of the tree -> lanes, depth levels -> steps.  `out` stays empty when
// the model does not fit a lane group (the one-lane generic kernel runs it): that is no error.
int build_tree_tab(const grx_config& c, const GenTables& T, const std::vector<int>& pos_of, int G, std::unique_ptr<TreeTab>& out) {
    const grx_model& m = c.model;
    const auto no_table = [&] { out.reset(); return (int)GRX_OK; };
    std::unique_ptr<TreeTab> tt(new TreeTab());
    TreeTab& K = *tt;
    memset(&K, 0, sizeof K);
    K.g = G;
    K.nb = T.nb; K.nd = T.nd; K.nsph = T.nsph; K.nlc = T.nlc;
    memset(K.sched, 0xff, sizeof K.sched);
    std::vector<int> depth(T.nb, -1), lane_of(T.nb, -1), cont(T.nb, 0);
    int nchain = 0, nstep = 0;
    bool fits = true;
    for (int b = 1; b < T.nb && fits; ++b) {
        const int p = T.parent[b];
        depth[b] = p == 0 ? 0 : depth[p] + 1;
        TreeBody& tb = K.body[b];
        bool head = false;
        if (p != 0 && !cont[p]) { lane_of[b] = lane_of[p]; cont[p] = 1; }   // a body's first child continues its chain
        else { head = true; lane_of[b] = nchain++; }
        if (nchain > GRX_TREE_G || depth[b] >= GRX_TREE_LEVELS) { fits = false; break; }
        if (head && p == 0) K.heads0[K.nh0++] = lane_of[b];
        if (head && p != 0) { if (K.body[p].nhc >= 4) { fits = false; break; } K.body[p].hc[K.body[p].nhc++] = lane_of[b]; }
        K.sched[lane_of[b]][depth[b]] = (int8_t)b;
        nstep = std::max(nstep, depth[b] + 1);
        for (int a = 0; a < 3; ++a) { tb.axis[a] = T.axis[b][a]; tb.jpos[a] = T.jpos[b][a]; tb.com[a] = T.com[b][a]; }
        for (int a = 0; a < 9; ++a) tb.rot0[a] = T.rot0[b][a];
        for (int a = 0; a < 6; ++a) tb.Ic[a] = T.Ic[b][a];
        tb.mass = T.mass[b]; tb.parent = p; tb.sph_begin = T.sph_begin[b]; tb.sph_end = T.sph_begin[b + 1];
        tb.lane = lane_of[b]; tb.step = depth[b];
        tb.rot0_identity = 1;
        for (int a = 0; a < 9; ++a) if (tb.rot0[a] != ((a % 4 == 0) ? 1.f : 0.f)) tb.rot0_identity = 0;
    }
    if (!fits) return no_table();   // more chains / levels than a lane group holds: the one-lane generic kernel runs it
    K.nchain = nchain; K.nstep = nstep;
    K.nstep_kin = 0;   // (the arms of the full body hang four levels deeper than anything the env pipeline reads)
    for (int b : {T.foot_body[0], T.foot_body[1], T.torso_body, T.forehead_body}) if (b >= 1) K.nstep_kin = std::max(K.nstep_kin, depth[b] + 1);
    for (int c = 0; c < GRX_TREE_GMAX; ++c) {
        K.first[c] = 1; K.last[c] = 0;
        bool any = false;
        for (int g = 0; g < nstep; ++g) if (K.sched[c][g] >= 0) { if (!any) K.first[c] = g; K.last[c] = g; any = true; }
    }
    for (int j = 0; j < T.nd; ++j) {
        TreeDof& d = K.dof[j];
        d.kp = T.kp[j]; d.kd = T.kd[j]; d.q0 = T.q0[j]; d.effort = T.effort[j]; d.vlim = T.vlim[j]; d.qlo = T.qlo[j]; d.qhi = T.qhi[j];
        d.slo = T.slo[j]; d.shi = T.shi[j]; d.amin = T.amin[j]; d.amax = T.amax[j]; d.Klim = T.Klim[j]; d.Clim = T.Clim[j]; d.lane = lane_of[j + 1]; d.arm = T.arm[j];
    }
    for (int k = 0; k < T.nsph; ++k) { TreeSph& q = K.sph[k]; q.x = T.sx[k]; q.y = T.sy[k]; q.z = T.sz[k]; q.r = T.sr[k]; q.dmax = T.sdmax[k]; q.slot = T.sslot[k]; q.link = T.slink[k]; }
    for (int l = 0; l < T.nlc; ++l) { K.link_flags[l] = T.link_flags[l]; K.link_urdf[l] = T.link_urdf[l]; }
    for (int f = 0; f < 2; ++f) { K.foot_body[f] = T.foot_body[f]; K.foot_link[f] = T.foot_link[f]; for (int a = 0; a < 3; ++a) K.foot_pos[f][a] = T.foot_pos[f][a]; }
    K.torso_body = T.torso_body; K.forehead_body = T.forehead_body;
    memcpy(K.torso_rot, T.torso_rot, sizeof K.torso_rot); memcpy(K.forehead_rot, T.forehead_rot, sizeof K.forehead_rot);
    K.sph_begin0 = T.sph_begin[0]; K.sph_end0 = T.sph_begin[1];
    {   // the contact pass's work list (TreeTab.cw): every body's shapes in chunks of two, the largest bodies first, dealt to the eight
        // lanes round by round; chunks of one body that land in the same round take turns at its accumulators.  A foot body is listed
        // even without shapes (its frame gives the sub-step averaged foot speed).
        struct Item { int body, s0, s1, turn; };
        std::vector<Item> items;
        std::vector<int> order;
        for (int b = 0; b < T.nb; ++b) order.push_back(b);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b_) { return (T.sph_begin[a + 1] - T.sph_begin[a]) > (T.sph_begin[b_ + 1] - T.sph_begin[b_]); });
        for (int b : order) {
            const int n0 = T.sph_begin[b], n1 = T.sph_begin[b + 1];
            const bool foot = b == T.foot_body[0] || b == T.foot_body[1];
            if (n1 == n0 && foot) items.push_back({b, n0, n0, 0});
            for (int i = n0; i < n1; i += 2) items.push_back({b, i, std::min(i + 2, n1), 0});
        }
        if (T.foot_body[0] < 1 || T.foot_body[1] < 1) return no_table();   // (feet on the base: not this kernel's layout)
        const int rounds = ((int)items.size() + G - 1) / G;
        if (rounds > GRX_TREE_MAXCS) return no_table();   // (the generic kernel runs it)
        memset(K.cw, 0xff, sizeof K.cw);
        K.ncs = rounds; K.nturn = 1;
        for (int r = 0; r < rounds; ++r)
            for (int ln = 0; ln < G; ++ln) {
                const size_t k = (size_t)r * G + ln;
                if (k >= items.size()) continue;
                Item it = items[k];
                for (int l2 = 0; l2 < ln; ++l2) if (K.cw[r][l2].body == it.body) it.turn = std::max(it.turn, K.cw[r][l2].turn + 1);
                K.cw[r][ln].body = (int8_t)it.body; K.cw[r][ln].s0 = (int8_t)it.s0; K.cw[r][ln].s1 = (int8_t)it.s1; K.cw[r][ln].turn = (int8_t)it.turn;
                K.nturn = std::max(K.nturn, it.turn + 1);
            }
    }
    K.nlp = T.nlp;
    for (int q = 0; q < T.nlp; ++q) { K.lp_ba[q] = (int16_t)T.lp_ba[q]; K.lp_bb[q] = (int16_t)T.lp_bb[q]; K.lp_a[q] = (int16_t)T.lp_a[q]; K.lp_b[q] = (int16_t)T.lp_b[q]; }
    {   // the broad phase's sphere pairs: every pair of grx_model.pair_a/b with its link pair; (ra + rb + margin)^2 -- the margin (0.1 mm) keeps the
        // test on the contact pass's centres a superset of sphere_pair's own (the two form a centre with differently rounded products)
        if (T.nsph > 255) return no_table();
        K.nsp = 0;
        for (int pi = 0; pi < m.num_pairs; ++pi) {
            int ka = pos_of[m.pair_a[pi]], kb = pos_of[m.pair_b[pi]];
            int la = T.slink[ka], lb = T.slink[kb];
            int lp = -1;
            for (int q = 0; q < T.nlp; ++q) if ((T.lp_a[q] == la && T.lp_b[q] == lb) || (T.lp_a[q] == lb && T.lp_b[q] == la)) lp = q;
            if (lp < 0) return fail(GRX_ERR_INVALID_ARGUMENT, "self-collision sphere pair without a link pair");
            const float rs = T.sr[ka] + T.sr[kb] + 1e-4f;
            K.sp[K.nsp].ab = (uint32_t)ka | ((uint32_t)kb << 8) | ((uint32_t)lp << 16);
            K.sp[K.nsp].r2 = rs * rs;
            ++K.nsp;
        }
        // the broad phase takes the table four rounds of the group's lanes at a time, without a bounds test: padded with pairs that never pass
        K.nsp_batches = (K.nsp + 4 * G - 1) / (4 * G);
        if (K.nsp_batches * 4 * G > GRX_MAX_PAIRS) return no_table();
        for (int k = K.nsp; k < K.nsp_batches * 4 * G; ++k) { K.sp[k].ab = 0u; K.sp[k].r2 = -1.f; }
    }
    for (int l = 0; l <= GEN_MAXLC; ++l) K.lc_begin[l] = T.lc_begin[l];
    out = std::move(tt);
    return GRX_OK;
}

// every URDF link frame by carrying body (grx_create has checked num_links and link_body)
void build_link_tab(const grx_model& m, LinkTab& lt) {
    memset(&lt, 0, sizeof lt);
    lt.n = m.num_links;
    for (int l = 0; l < m.num_links; ++l) {
        lt.body[l] = m.link_body[l];
        for (int a = 0; a < 3; ++a) lt.pos[l][a] = m.link_pos[l][a];
        for (int a = 0; a < 9; ++a) lt.rot[l][a] = m.link_rot[l][a];
    }
}

// grx_refresh: the joint tree as the model holds it.  false: a tree deeper than the refresh kernel walks (such models run on the one-lane generic kernel)
bool build_refresh_tab(const grx_model& m, RefreshTab& rt) {
    memset(&rt, 0, sizeof rt);
    rt.nb = m.num_bodies; rt.nlinks = m.num_links;
    for (int b = 1; b < m.num_bodies; ++b) {
        int n = 0;
        for (int x = b; x > 0 && n <= GRX_MAX_BODIES; x = m.parent[x]) ++n;
        if (n > GRX_REFRESH_MAXDEPTH) return false;
    }
    for (int b = 1; b < m.num_bodies; ++b) {
        int chain[GRX_MAX_BODIES], n = 0;
        for (int x = b; x > 0 && n < GRX_MAX_BODIES; x = m.parent[x]) chain[n++] = x;
        rt.depth[b] = n;
        for (int d = 0; d < n; ++d) rt.path[b][d] = (int8_t)chain[n - 1 - d];
        bool ident = true;
        for (int a = 0; a < 9; ++a) { rt.rot0[b][a] = m.joint_rot0[b][a]; ident = ident && m.joint_rot0[b][a] == (a % 4 == 0 ? 1.f : 0.f); }
        rt.rot0_identity[b] = ident ? 1 : 0;
        for (int a = 0; a < 3; ++a) { rt.axis[b][a] = m.joint_axis[b][a]; rt.jpos[b][a] = m.joint_pos[b][a]; }
    }
    return true;
}

// ---- the raster of a heightfield terrain as the kernels read it
struct TerrainTables {
    std::vector<uint32_t> cells;   // KParams::hf_cells, two words per cell; mesh_type 'trimesh': the corrected mesh's tables behind them, from cell tm_off on
    std::vector<int16_t> max4;     // KParams::hf_max4
    std::vector<float> coarse;     // KParams::coarse_max [coarse_rows][coarse_cols]
    size_t tm_off = 0;
    int coarse_rows = 0, coarse_cols = 0;
};
TerrainTables build_terrain_tables(const grx_config& c) {
    TerrainTables out;
    const size_t n = (size_t)c.hf_rows * c.hf_cols;
    const bool vertical_faces = c.vertical_faces != 0;
    // per-cell max of the four corners the bilinear terrain query blends (terrain_height in grx_kernels.hip)
    out.max4.resize(n);
    for (int i = 0; i < c.hf_rows; ++i)
        for (int j = 0; j < c.hf_cols; ++j) {
            const int i1 = std::min(i + 1, c.hf_rows - 1), j1 = std::min(j + 1, c.hf_cols - 1);
            const int16_t* H = c.height_samples;
            out.max4[(size_t)i * c.hf_cols + j] = std::max(std::max(H[(size_t)i * c.hf_cols + j], H[(size_t)i1 * c.hf_cols + j]),
                                                           std::max(H[(size_t)i * c.hf_cols + j1], H[(size_t)i1 * c.hf_cols + j1]));
        }
    {   // the four corners of every cell, packed (grx_device.h hf_cells); mesh_type 'trimesh': + the corrected mesh's tables behind them
        const size_t tm_off = vertical_faces ? ((n + 1) & ~(size_t)1) : 0;
        out.cells.assign(2 * (vertical_faces ? 3 * tm_off + 2 * n : n), 0u);
        for (int i = 0; i < c.hf_rows; ++i)
            for (int j = 0; j < c.hf_cols; ++j) {
                const int i1 = std::min(i + 1, c.hf_rows - 1), j1 = std::min(j + 1, c.hf_cols - 1);
                const int16_t* H = c.height_samples;
                const uint32_t h00 = (uint16_t)H[(size_t)i * c.hf_cols + j], h01 = (uint16_t)H[(size_t)i * c.hf_cols + j1];
                const uint32_t h10 = (uint16_t)H[(size_t)i1 * c.hf_cols + j], h11 = (uint16_t)H[(size_t)i1 * c.hf_cols + j1];
                out.cells[2 * ((size_t)i * c.hf_cols + j)] = h00 | (h01 << 16);
                out.cells[2 * ((size_t)i * c.hf_cols + j) + 1] = h10 | (h11 << 16);
            }
        if (vertical_faces) {
            TrimeshTables tm = build_trimesh_tables(c);
            for (size_t k = 0; k < n; ++k) {
                const int16_t* e = &tm.ground[6 * k];
                uint32_t* t0 = &out.cells[2 * (tm_off + 2 * k)];
                t0[0] = (uint16_t)e[0] | ((uint32_t)(uint16_t)e[1] << 16); t0[1] = (uint16_t)e[2];
                t0[2] = (uint16_t)e[3] | ((uint32_t)(uint16_t)e[4] << 16); t0[3] = (uint16_t)e[5];
                const int16_t* w = &tm.walls[8 * k];
                uint32_t* w0 = &out.cells[2 * (3 * tm_off + 2 * k)];
                for (int q = 0; q < 4; ++q) w0[q] = (uint16_t)w[2 * q] | ((uint32_t)(uint16_t)w[2 * q + 1] << 16);
                int16_t top = out.max4[k];   // the contact reach test (grx_rare.h) must see what the cell can touch: its ground corners and its faces' tops
                for (int q = 0; q < 6; ++q) top = std::max(top, e[q]);
                for (int q = 0; q < 8; ++q) top = std::max(top, w[q]);
                out.max4[k] = top;
            }
            out.tm_off = tm_off;
        }
    }
    {   // coarse max map: max height over each 8x8-cell block dilated by 3 blocks (>= 2.4 m: robot reach 1.1 m
        // + travel within a policy step + bilinear support), used only to cull spheres that cannot touch
        int cr = (c.hf_rows + GRX_COARSE - 1) / GRX_COARSE, cc = (c.hf_cols + GRX_COARSE - 1) / GRX_COARSE;
        std::vector<int16_t> blk((size_t)cr * cc, INT16_MIN);
        for (int i = 0; i < c.hf_rows; ++i)
            for (int j = 0; j < c.hf_cols; ++j) {
                int16_t& b = blk[(size_t)(i / GRX_COARSE) * cc + j / GRX_COARSE];
                int16_t v = c.height_samples[(size_t)i * c.hf_cols + j];
                if (v > b) b = v;
            }
        out.coarse.resize((size_t)cr * cc);
        for (int i = 0; i < cr; ++i)
            for (int j = 0; j < cc; ++j) {
                int16_t m = INT16_MIN;
                for (int di = -3; di <= 3; ++di)
                    for (int dj = -3; dj <= 3; ++dj) {
                        int ii = i + di, jj = j + dj;
                        if (ii < 0 || jj < 0 || ii >= cr || jj >= cc) continue;
                        if (blk[(size_t)ii * cc + jj] > m) m = blk[(size_t)ii * cc + jj];
                    }
                out.coarse[(size_t)i * cc + j] = (float)m * c.vertical_scale;
            }
        out.coarse_rows = cr; out.coarse_cols = cc;
    }
    return out;
}

// ---- per-env constants on the host (same arithmetic as the oracle's gro_create): SoA [k][N] like the device buffers they fill
struct EnvConstants {
    std::vector<float> motor_strength, base_m, base_c, base_I, friction, restitution, origins, q, root;
    std::vector<float> base_mass_com;   // GRX_T_BASE_MASS_COM, (N, 4) row-major
    std::vector<int32_t> levels, types;
    std::vector<uint8_t> reset;
};
EnvConstants build_env_constants(const grx_config& c) {
    const grx_model& m = c.model;
    const size_t N = (size_t)c.num_envs;
    const int nd = m.num_bodies - 1;
    EnvConstants E;
    E.motor_strength.resize(nd * N); E.base_m.resize(N); E.base_c.resize(3 * N); E.base_I.resize(6 * N); E.friction.resize(N); E.restitution.resize(N);
    E.origins.resize(3 * N); E.q.resize(nd * N); E.root.assign(13 * N, 0.f); E.base_mass_com.resize(4 * N);
    E.levels.assign(N, 0); E.types.assign(N, 0);
    E.reset.assign(N, 1);
    for (size_t i = 0; i < N; ++i) {
        uint32_t ge = (uint32_t)(c.env_offset + (int)i);
        float origin[3] = {0, 0, 0};
        if (c.terrain_type == GRX_TERRAIN_HEIGHTFIELD) {
            int max_init = c.curriculum ? c.max_init_terrain_level : c.num_terrain_rows - 1;
            float u = grx_rand(c.seed, ge, 0, GRX_RNG_INIT_LEVEL, 0);
            int lv = (int)(u * (float)(max_init + 1));
            if (lv > max_init) lv = max_init;
            // torch.div(arange(N), N / num_cols, rounding_mode='floor') evaluates in float32 (legged_robot.py:1177-1180)
            float per = (float)((double)c.total_envs / c.num_terrain_cols);
            int ty = (int)torch_div_floor((float)ge, per);
            if (ty > c.num_terrain_cols - 1) ty = c.num_terrain_cols - 1;
            E.levels[i] = lv; E.types[i] = ty;
            const float* o = c.terrain_origins + ((size_t)lv * c.num_terrain_cols + ty) * 3;
            origin[0] = o[0]; origin[1] = o[1]; origin[2] = o[2];
        } else {
            int ncols = (int)floor(sqrt((double)c.total_envs));
            if (ncols < 1) ncols = 1;
            origin[0] = c.env_spacing * (float)(ge / (uint32_t)ncols);
            origin[1] = c.env_spacing * (float)(ge % (uint32_t)ncols);
        }
        for (int k = 0; k < 3; ++k) E.origins[k * N + i] = origin[k];
        float fr = 1.f;
        if (c.randomize_friction) {
            uint32_t b = (uint32_t)(grx_rand(c.seed, ge, 0, GRX_RNG_INIT_DR, 0) * 64);
            if (b > 63) b = 63;
            fr = c.friction_range[0] + (c.friction_range[1] - c.friction_range[0]) * grx_rand(c.seed, b, 1, GRX_RNG_INIT_DR, 0);
        }
        E.friction[i] = fr;
        float rs = 0.f;
        if (c.randomize_restitution) {
            uint32_t b = (uint32_t)(grx_rand(c.seed, ge, 0, GRX_RNG_INIT_DR, 1) * 64);
            if (b > 63) b = 63;
            rs = c.restitution_range[0] + (c.restitution_range[1] - c.restitution_range[0]) * grx_rand(c.seed, b, 1, GRX_RNG_INIT_DR, 1);
        }
        E.restitution[i] = rs;
        float lm = m.base_link_mass, lc[3] = {m.base_link_com[0], m.base_link_com[1], m.base_link_com[2]};
        if (c.randomize_base_mass) lm *= c.base_mass_range[0] + (c.base_mass_range[1] - c.base_mass_range[0]) * grx_rand(c.seed, ge, 0, GRX_RNG_INIT_DR, 2);
        if (c.randomize_base_com)
            for (int k = 0; k < 3; ++k) lc[k] += c.base_com_range[k][0] + (c.base_com_range[k][1] - c.base_com_range[k][0]) * grx_rand(c.seed, ge, 0, GRX_RNG_INIT_DR, 3 + k);
        float M, cc[3], I6[6];
        base_lump(m, lm, lc, &M, cc, I6);
        E.base_m[i] = M;
        for (int k = 0; k < 3; ++k) E.base_c[k * N + i] = cc[k];
        for (int k = 0; k < 6; ++k) E.base_I[k * N + i] = I6[k];
        E.base_mass_com[4 * i] = lm;
        for (int k = 0; k < 3; ++k) E.base_mass_com[4 * i + 1 + k] = lc[k];
        for (int j = 0; j < nd; ++j) {
            float st = 1.f;
            if (c.randomize_motor_strength) st = c.motor_strength_range[0] + (c.motor_strength_range[1] - c.motor_strength_range[0]) * grx_rand(c.seed, ge, 0, GRX_RNG_INIT_DR, 8 + j);
            E.motor_strength[j * N + i] = st;
            E.q[j * N + i] = c.default_dof_pos[j];
        }
        for (int k = 0; k < 3; ++k) E.root[k * N + i] = c.init_pos[k] + origin[k];
        E.root[6 * N + i] = 1.f;
    }
    return E;
}

// ---- the scalar launch parameters: grx_config -> KParams, environment overrides included (the pointers and what depends on the layout: grx_create)
void fill_params(const grx_config& c, KParams& P) {
    const grx_model& m = c.model;
    const int nd = m.num_bodies - 1, nh = c.measure_heights ? c.num_height_points : 0;
    memset(&P, 0, sizeof P);
    P.N = c.num_envs; P.env_offset = c.env_offset; P.total_envs = c.total_envs; P.nd = nd;
    const char* dbg = getenv("GRX_PUBLISH_DEBUG");   // (tools/: overrides the config either way)
    P.publish_debug = dbg ? atoi(dbg) : c.publish_reward_terms;
    P.seed = c.seed;
    P.sim_dt = c.sim_dt; P.decimation = c.decimation;
    for (int i = 0; i < 3; ++i) { P.gravity[i] = c.gravity[i]; P.init_pos[i] = c.init_pos[i]; }
    P.action_scale = c.action_scale;
    P.control_type = c.control_type; P.heading_command = c.heading_command ? 1 : 0;
    P.kn = c.contact.kn; P.dn = c.contact.dn; P.kt = c.contact.kt; P.ct = c.contact.ct; P.cv = c.contact.cv;
    P.terrain_friction = c.contact.terrain_friction;
    P.inv_kt = 1.0f / c.contact.kt;
    P.bounce_threshold = c.bounce_threshold_velocity; P.terrain_restitution = c.terrain_restitution;
    P.self_collisions = c.self_collisions;
    if (const char* sc = getenv("GRX_SELF_COLLISIONS")) P.self_collisions = atoi(sc);   // A/B runs (tools/)
    if (getenv("GRX_NO_RESTITUTION")) P.bounce_threshold = 1e30f;   // A/B runs: no contact ever bounces (tools/train_ab.py)
    P.termination_force = c.termination_force; P.termination_gravity_z = c.termination_gravity_z;
    P.max_episode_length = c.max_episode_length; P.max_episode_length_s = c.max_episode_length_s;
    P.resample_command_interval = c.resample_command_interval;
    for (int i = 0; i < 2; ++i) { P.cmd_lin_vel_x[i] = c.cmd_lin_vel_x[i]; P.cmd_lin_vel_y[i] = c.cmd_lin_vel_y[i]; P.cmd_ang_vel_yaw[i] = c.cmd_ang_vel_yaw[i]; }
    P.randomize_init_dof_pos = c.randomize_init_dof_pos; P.randomize_init_base_velocity = c.randomize_init_base_velocity;
    P.push_robots = c.push_robots; P.push_interval = c.push_interval; P.max_push_vel_xy = c.max_push_vel_xy;
    const float dtp = c.sim_dt * (float)c.decimation;
    for (int t = 0; t < NT; ++t) { P.reward_scale_dt[t] = c.reward_scale[t] * dtp; P.reward_sigma[t] = c.reward_sigma[t]; }
    P.only_positive_rewards = c.only_positive_rewards;
    for (int t = 0; t < GRX_NUM_BASE_REWARD_TERMS; ++t) { P.base_scale_dt[t] = c.base_reward_scale[t] * dtp; if (c.base_reward_scale[t] != 0.f) P.base_active |= 1u << t; }
    P.tracking_sigma = c.tracking_sigma; P.max_contact_force = c.max_contact_force;
    P.command_curriculum = c.command_curriculum ? 1 : 0; P.max_curriculum = c.max_curriculum;
    P.base_height_target = c.base_height_target; P.swing_feet_height_target = c.swing_feet_height_target;
    P.feet_stumble_ratio = c.feet_stumble_ratio; P.feet_air_time_target = c.feet_air_time_target; P.feet_land_time_max = c.feet_land_time_max;
    P.soft_dof_vel_limit = c.soft_dof_vel_limit; P.soft_torque_limit = c.soft_torque_limit;
    P.knee_mask = c.knee_mask; P.hip_roll_mask = c.hip_roll_mask; P.hip_yaw_mask = c.hip_yaw_mask;
    P.ankle_left_mask = c.ankle_left_mask; P.ankle_right_mask = c.ankle_right_mask;
    P.num_pri_obs = c.num_pri_obs;
    P.obs_scale_action = c.obs_scale_action; P.obs_scale_lin_vel = c.obs_scale_lin_vel; P.obs_scale_ang_vel = c.obs_scale_ang_vel;
    P.obs_scale_gravity = c.obs_scale_gravity; P.obs_scale_dof_pos = c.obs_scale_dof_pos; P.obs_scale_dof_vel = c.obs_scale_dof_vel;
    P.obs_scale_height = c.obs_scale_height;
    P.add_noise = c.add_noise; P.noise_level = c.noise_level; P.noise_action = c.noise_action; P.noise_ang_vel = c.noise_ang_vel;
    P.noise_gravity = c.noise_gravity; P.noise_dof_pos = c.noise_dof_pos; P.noise_dof_vel = c.noise_dof_vel;
    P.clip_observations = c.clip_observations;
    P.terrain_type = c.terrain_type; P.measure_heights = c.measure_heights; P.nh = nh;
    P.hf_rows = c.hf_rows; P.hf_cols = c.hf_cols;
    P.horizontal_scale = c.horizontal_scale; P.vertical_scale = c.vertical_scale; P.border_size = c.border_size;
    P.inv_hscale = 1.0f / c.horizontal_scale;
    P.vertical_faces = c.terrain_type == GRX_TERRAIN_HEIGHTFIELD && c.vertical_faces; P.tm_off = 0;   // (tm_off: with the cell tables, grx_create)
    P.hv_scale = c.vertical_scale / c.horizontal_scale;
    P.curriculum = c.curriculum; P.num_terrain_rows = c.num_terrain_rows; P.num_terrain_cols = c.num_terrain_cols;
    P.terrain_length = c.terrain_length;
    memcpy(P.torso_rot, m.torso_rot, sizeof P.torso_rot);
    memcpy(P.forehead_rot, m.forehead_rot, sizeof P.forehead_rot);
    P.has_torso = m.torso_body >= 0; P.has_forehead = m.forehead_body >= 0;
    P.num_links = m.num_links;
}
}  // namespace
