// grx_gen_tables.h -- GenTables alone: the generic-tree kernels' model tables.  ONE text for both sides: grx_generic.h includes it where the struct
// stands (inside grx_kernels.hip's anonymous namespace: the kernels' mangled names carry the type from there), grx_host_tables.h inside the host
// translation unit's own.  The limits GEN_MAXLC / GEN_MAXLP: grx_device.h.
constexpr int GEN_MAXB = GRX_MAX_BODIES, GEN_MAXD = GRX_MAX_DOFS, GEN_MAXS = GRX_MAX_SPHERES;
struct GenTables {
    int32_t nb, nd, nsph, nlc;
    int32_t parent[GEN_MAXB];
    float axis[GEN_MAXB][3], rot0[GEN_MAXB][9], jpos[GEN_MAXB][3], mass[GEN_MAXB], com[GEN_MAXB][3], Ic[GEN_MAXB][6];
    float kp[GEN_MAXD], kd[GEN_MAXD], q0[GEN_MAXD], effort[GEN_MAXD], vlim[GEN_MAXD], qlo[GEN_MAXD], qhi[GEN_MAXD];
    float slo[GEN_MAXD], shi[GEN_MAXD], amin[GEN_MAXD], amax[GEN_MAXD], Klim[GEN_MAXD], Clim[GEN_MAXD];
    float arm[GEN_MAXD];               // joint-space armature (grx_model.dof_armature)
    int32_t sph_begin[GEN_MAXB + 1];   // spheres are sorted by carrying body
    float sx[GEN_MAXS], sy[GEN_MAXS], sz[GEN_MAXS], sr[GEN_MAXS], sdmax[GEN_MAXS];
    int32_t sslot[GEN_MAXS];           // friction-anchor slot 0..7 of an anchored foot sphere, -1 otherwise
    int32_t slink[GEN_MAXS];           // compact id of the URDF link the shape belongs to (force netting)
    uint32_t link_flags[GEN_MAXLC];    // GRX_SPH_TERMINATE / GRX_SPH_PENALISE of the compact links
    int32_t link_urdf[GEN_MAXLC];      // URDF link index of the compact links (row of GRX_T_CONTACT_FORCES)
    int32_t foot_body[2], foot_link[2];
    float foot_pos[2][3];
    int32_t torso_body, forehead_body;
    float torso_rot[9], forehead_rot[9];
    // self-collision (grx_model.pair_a / pair_b grouped by link pair): compact links a, b on bodies ba, bb, bounding
    // spheres of their shapes (body frame: xyz, radius); a compact link's shapes are sx[lc_begin[l] .. lc_begin[l + 1])
    int32_t nlp;
    int32_t lp_a[GEN_MAXLP], lp_b[GEN_MAXLP], lp_ba[GEN_MAXLP], lp_bb[GEN_MAXLP];
    float lp_ca[GEN_MAXLP][4], lp_cb[GEN_MAXLP][4];
    int32_t lc_begin[GEN_MAXLC + 1];
};
// both sides compile this line too: a side that saw other limits (GRX_MAX_*, GEN_MAX*) does not build
static_assert(sizeof(GenTables) == 9764, "GenTables: the kernels and the host must see one layout");
