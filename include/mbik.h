/*
 * mbik.h -- C ABI of the MI355X-native batched many-bone IK solver.
 *
 * Drop-in boundary for the per-frame solve path of Ughuuu/many_bone_ik
 * (snapshot 2024-08-07).  Each entry point names the reference interface it replaces:
 *
 *   mbik_plan_create   <- ManyBoneIK3D::_bone_list_changed()      src/many_bone_ik_3d.cpp:1011-1068
 *                         (segmentation, heading weights, bone directions, Kusudama setup;
 *                          IKBoneSegment3D::generate_default_segments ik_bone_segment_3d.cpp:352-427,
 *                          IKBone3D::update_default_bone_direction_transform ik_bone_3d.cpp:57-93,
 *                          IKLimitCone3D::update_tangent_handles ik_open_cone_3d.cpp:36-120,
 *                          IKKusudama3D::set_axial_limits/_update_constraint ik_kusudama_3d.cpp:37-115)
 *   mbik_solve         <- ManyBoneIK3D::_process_modification()   src/many_bone_ik_3d.cpp:645-694
 *                         (the virtual SkeletonModifier3D hook, many_bone_ik_3d.h:90; preceded by
 *                          _update_ik_bones_transform :91-102 and followed by
 *                          _update_skeleton_bones_transform :104-116), for a batch of skeletons
 *   mbik_solve_host    <- same, synchronous, host buffers
 *   mbik_segment_solve <- IKBoneSegment3D::segment_solver()       src/ik_bone_segment_3d.cpp:210-225
 *                         (one call = one segment_solver() of one segment subtree)
 *   mbik_pose_globals  <- Skeleton3D::get_bone_global_pose for every bone, as the reference calls
 *                         it at src/ik_bone_3d.cpp:71 (and global * bind_inverse for skinning)
 *   mbik_pose_blend    <- Skeleton3D::_process_modifiers' blend of the poses before and after a
 *                         SkeletonModifier3D by its inherited `influence` property (Godot 4.3 core)
 *   mbik_clip_sample   <- Animation::position_track_interpolate / rotation_track_interpolate /
 *                         scale_track_interpolate for every bone: the animation that writes the poses
 *                         a SkeletonModifier3D receives (Godot 4.3 core)
 *   mbik_clip_sample_layers <- AnimationMixer::_blend_process / _blend_apply: the blend of several
 *                         animations, each with its own time and weight (Godot 4.3 core)
 *   mbik_plan_destroy  <- ~ManyBoneIK3D / set_dirty() rebuild
 *   mbik_last_error    <- ERR_FAIL_* messages (the reference prints and returns)
 *
 * Plain pointers and sizes only.  All float arrays are float32, row-major, one skeleton
 * after another:
 *   pose    [skel][bone][10]  quaternion x,y,z,w | position x,y,z | scale x,y,z
 *                             (Skeleton3D bone pose; ik_bone_3d.cpp:161-179)
 *   target  [skel][pin][12]   basis rows r0,r1,r2 | origin, in skeleton space
 *                             (IKEffector3D::target_relative_to_skeleton_origin, ik_effector_3d.cpp:77-84)
 *   cones   [skel][constraint][max_cones][4]  centre x,y,z | radius (kusudama_open_cones)
 *   twist   [skel][constraint][2]             from, range (joint_twist)
 *
 * Threading: a plan is not thread-safe; distinct plans may be used concurrently on
 * distinct streams.  mbik_solve is asynchronous on the given HIP stream.
 * Errors: 0 on success, a negative MBIK_E* code otherwise; mbik_last_error() explains.
 * Non-finite output bases become identity rotations, as ik_bone_3d.cpp:174-176 does.
 */
#ifndef MBIK_H
#define MBIK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBIK_OK 0
#define MBIK_EINVAL (-1)
#define MBIK_ENOMEM (-2)
#define MBIK_EHIP (-3)
#define MBIK_EUNSUPPORTED (-4)
#define MBIK_ENODEV (-5)

#define MBIK_ABI_VERSION 15

typedef struct mbik_plan mbik_plan;
typedef struct mbik_group mbik_group;
typedef struct mbik_multi mbik_multi;

/* == IKEffectorTemplate3D (src/ik_effector_template_3d.h:40-47). */
typedef struct mbik_pin {
	int32_t bone;                      /* skeleton bone index (template name) */
	float weight;                      /* reference default 0.0 */
	float direction_priorities[3];     /* reference default (0.2, 0, 0.2) */
	float motion_propagation_factor;   /* reference default 1.0, clamped to [0,1] */
} mbik_pin;

/* == one ManyBoneIK3D "constraints/<i>" entry (many_bone_ik_3d.cpp:1037-1067). */
typedef struct mbik_constraint {
	int32_t bone;                      /* constraint_names[i] resolved to a bone index */
	int32_t cone_count;                /* kusudama_open_cone_count[i] */
} mbik_constraint;

typedef struct mbik_skeleton_desc {
	int32_t bone_count;
	const int32_t *parents;            /* [bone_count]; -1 = parentless */
	int32_t pin_count;
	const mbik_pin *pins;
	int32_t constraint_count;
	const mbik_constraint *constraints;
	int32_t max_cones;                 /* stride of the cones array */
} mbik_skeleton_desc;

/* ManyBoneIK3D solver properties (many_bone_ik_3d.h:49-68). */
typedef struct mbik_config {
	int32_t iterations_per_frame;      /* reference default 15 */
	float default_damp;                /* radians; reference default deg_to_rad(5) */
	int32_t constraint_mode;           /* reference default false */
	int32_t stabilization_passes;      /* reference default 0 */
	int32_t bone_damp_count;           /* ManyBoneIK3D::bone_damp, usually empty */
	const float *bone_damp;
} mbik_config;

typedef struct mbik_plan_info {
	int32_t abi_version;
	int32_t skeleton_count;
	int32_t bone_count;
	int32_t pin_count;
	int32_t segment_count;
	int32_t level_count;               /* sibling-segment levels solved concurrently */
	int32_t lanes_per_skeleton;
	int32_t skeletons_per_block;
	int32_t max_headings;
	int32_t device;
	int64_t device_bytes;              /* per-skeleton plan tables resident in HBM */
	double algorithmic_bytes_per_skeleton; /* per bone pose in/out 80 B + bone-direction quaternion 16 B + damp 4 B; per effector 64 B; per constrained bone 52 B + 52 B per cone (C2 8,292 B) */
	double algorithmic_flops_per_skeleton; /* SURVEY.md §8(d) per-bone-step formula x bone-steps x iterations */
	int64_t lds_bytes_per_block;       /* LDS of one launch block (spw skeletons + topology tables) */
	int32_t checkpoint_interval;       /* iteration-start globals kept every n-th bone (1 << 20: segment roots only) */
	int32_t heading_staging;           /* mbik_plan_set_heading_staging in effect (0 .. 5) */
	int32_t state_placement;           /* mbik_plan_set_locals_placement in effect (0 / 1 / 2) */
	int32_t waves_per_simd;            /* mbik_plan_set_waves_per_simd in effect (1 / 2) */
	int32_t constraint_slots;          /* slots of mbik_plan_setup_tables' CF / CD (ABI 3) */
	int32_t cf_stride;                 /* floats per slot of CF = 14 + 31*max_cones (ABI 3) */
	int32_t cd_stride;                 /* doubles per slot of CD = 2*max_cones (ABI 3) */
	int32_t libm_variant;              /* mbik_plan_options.libm_variant the plan was created with (ABI 4) */
	int32_t helper_wave;               /* 1 when the current layout launches with the helper wave (ABI 5) */
	int32_t heading_slots;             /* 0x67 when every effector has the reference's default direction
	                                      priorities (x, z > 0, y = 0: ik_effector_template_3d.h:45), so the
	                                      plan launches the kernels built for that heading set; 0 when the
	                                      priorities differ, and each effector's slots are tested at run
	                                      time (ABI 7).  Bits: 0 the origin heading, 1+2a and 2+2a the
	                                      +/- headings of axis a. */
	int32_t wave_roles;                /* 1 when the current layout runs with wave roles
	                                      (mbik_plan_set_wave_roles): lanes_per_skeleton is then the
	                                      number of waves per block (ABI 8) */
} mbik_plan_info;

/* Which reference host the plan reproduces bit for bit (ABI 4).  Godot's Math::sin/cos(float)
 * call the platform ::sinf/::cosf -- glibc on the reference's Linux x86-64 build -- and glibc
 * 2.35 ships two builds of them, picked per CPU by an ifunc; they differ on 12 (sinf) and 22
 * (cosf) of the 2^32 float inputs, and the solve amplifies a 1-ulp difference ~2x per
 * iteration, so the choice is part of the reference's behaviour:
 *   MBIK_LIBM_VARIANT_FMA   (0, default) the FMA build: a reference running on any x86-64
 *                           CPU with FMA (every Intel since Haswell, AMD since Piledriver;
 *                           the GPU boxes' EPYC 9575F);
 *   MBIK_LIBM_VARIANT_SSE2  (1) the SSE2 build: a reference on a CPU without FMA, or with the
 *                           ifunc disabled (GLIBC_TUNABLES=glibc.cpu.hwcaps=-FMA,-AVX2_Usable).
 * acosf has a single build.  The variant applies to the setup tables (cone and twist
 * half-angle sines/cosines, tangent frames) and to the solve's slerp coefficient. */
#define MBIK_LIBM_VARIANT_FMA 0
#define MBIK_LIBM_VARIANT_SSE2 1
typedef struct mbik_plan_options {
	int32_t struct_size;               /* sizeof(mbik_plan_options): later fields are optional */
	int32_t libm_variant;              /* MBIK_LIBM_VARIANT_* */
} mbik_plan_options;

/* Builds the per-topology tables and the per-skeleton setup data for skeletons
 * [0, n_skeletons) from their setup poses, uploads them to `device`.  cones/twist may be
 * NULL when constraint_count == 0. */
int32_t mbik_plan_create(const mbik_skeleton_desc *desc, const mbik_config *config, int32_t n_skeletons,
		const float *setup_pose, const float *cones, const float *twist, int32_t device, mbik_plan **out_plan);
/* mbik_plan_create with creation options (ABI 4; opts NULL = the defaults). */
int32_t mbik_plan_create_opts(const mbik_skeleton_desc *desc, const mbik_config *config, const mbik_plan_options *opts,
		int32_t n_skeletons, const float *setup_pose, const float *cones, const float *twist, int32_t device,
		mbik_plan **out_plan);
void mbik_plan_destroy(mbik_plan *plan);
/* Plan serialisation to a flat binary (checkpoint / resume, or a plan built once and shipped):
 * the creation inputs (topology, pins, constraints, config), the per-skeleton setup tables as
 * they are on the device (including any mbik_plan_rebuild_setup), the layout overrides and
 * autotune choice, and for constraint_mode the persistent node caches.  mbik_plan_save with
 * buf == NULL stores the needed size in *size; otherwise capacity must be at least that
 * (MBIK_EINVAL).  It reads the device tables back, so the streams using the plan must be
 * idle.  mbik_plan_load rebuilds the plan on `device` from such a buffer; the loaded plan
 * solves bitwise like the saved one.  Format version 5 (1-4 still load), little-endian,
 * host-independent. */
int32_t mbik_plan_save(const mbik_plan *plan, void *buf, uint64_t capacity, uint64_t *size);
int32_t mbik_plan_load(const void *buf, uint64_t size, int32_t device, mbik_plan **out_plan);
int32_t mbik_plan_get_info(const mbik_plan *plan, mbik_plan_info *out);
/* Launch-shape override (0 = automatic).  lanes_per_skeleton must be a power of two <= 64. */
int32_t mbik_plan_set_launch(mbik_plan *plan, int32_t lanes_per_skeleton);
/* Full layout override, each 0 = automatic: lanes per skeleton (power of two <= 64),
 * skeletons per block (<= 64 / lanes), and the checkpoint interval of the iteration-start
 * globals kept in LDS (1 = every bone; n = every n-th bone of a segment from its root, plus
 * the parents of segment roots).  Results do not depend on the layout. */
int32_t mbik_plan_set_layout(mbik_plan *plan, int32_t lanes_per_skeleton, int32_t skeletons_per_block,
		int32_t global_checkpoint_interval);
/* Heading staging of segments with several effectors (default 1): the lanes of the
 * segment's group split its effectors' heading builds and stage the QCP terms in LDS.  0:
 * every lane of the group solves the segment alone from registers -- no staging LDS, so
 * more skeletons fit per CU, at a longer step for those segments.  2: only the translating
 * root segments (the ones with the most effectors) are staged; 3: only segments with two or
 * more effectors (whose path walks the lanes split).
 * 4: split-exchange -- no segment is staged in memory; the lanes of a multi-effector segment's
 * group build alternate effectors' headings and read each other's through cross-lane
 * operations (ds_bpermute), every lane summing all of them in the reference's order; 5: the
 * translating root segments staged as in 2, the other multi-effector segments split-exchanged
 * as in 4.  Modes 4 and 5 are served by the two-waves-per-SIMD build only
 * (mbik_plan_set_waves_per_simd 2): with one wave per SIMD their split-exchange segments are
 * solved as in 0 (each lane alone); when the setup tables need 64-bit indices
 * (mbik_plan_set_table_addressing) 4 becomes 0 and 5 becomes 2, which
 * mbik_plan_info.heading_staging then reports.  -1: automatic (mbik_plan_autotune times them; it picks 4 for the
 * residency-bound BASELINE configs C3-C5).  Not used by constraint_mode (its lanes own tree
 * ranges).  Results do not depend on it. */
int32_t mbik_plan_set_heading_staging(mbik_plan *plan, int32_t staging);
/* Where the solve keeps its per-skeleton state during a launch: 0 (default) all in LDS;
 * 1 the bone local transforms in a per-skeleton device-memory area (L2-resident; about half
 * the LDS of a long-chain skeleton), the rest in LDS; 2 all of it in device memory (LDS holds
 * only the block's topology copy).  Less LDS per skeleton, more skeletons resident per CU.
 * -1: automatic (mbik_plan_autotune times each).  Results do not depend on it. */
int32_t mbik_plan_set_locals_placement(mbik_plan *plan, int32_t placement);
/* Waves per SIMD the solve kernel is built for: 1 (default) the whole register file; 2 at
 * most 256 registers (some spilled), so two blocks share a SIMD -- for launches too large to
 * be resident at once.  -1: automatic (mbik_plan_autotune times both).  Plans with
 * stabilization passes always use 1.  Results do not depend on it. */
int32_t mbik_plan_set_waves_per_simd(mbik_plan *plan, int32_t waves);
/* Helper wave: 1 launches two waves per block, on two SIMDs of a CU; the second runs the
 * global pass and computes each bone-step's parent-side work (the parent's global and its
 * inverse, the bone's global, the slerp's target side, the bone-direction and twist frames)
 * one step ahead of the solving wave, which then runs only what depends on the step's fit.
 * It pays where SIMDs would otherwise idle: launches resident at once with their state in LDS
 * (a frame of BASELINE configs[1]).  Serves state placement 0 without stabilization; other
 * layouts ignore it.  0 off, -1 (default) automatic: off until mbik_plan_autotune has timed
 * it on a fully resident launch.  Results do not depend on it.
 * Every wait between the two waves has an exit: a wait whose counter has not moved for two
 * seconds (a real wait lasts at most one iteration of the partner) gives up for the rest of
 * the launch.  The block's skeletons are then written as failures -- identity rotation, NaN
 * position, unit scale for every solved bone -- with their mbik_solve_checked flag set, and
 * the plan's own timeout flag is raised (mbik_plan_status).  The synchronous calls
 * (mbik_solve_host, mbik_plan_autotune) return MBIK_EHIP for their own launch; the
 * asynchronous ones (mbik_solve, mbik_solve_checked, mbik_segment_solve, mbik_group_solve)
 * return MBIK_EHIP, without launching, on the plan's next call, which clears the flag.
 * Plans never see each other's timeouts. */
int32_t mbik_plan_set_helper_wave(mbik_plan *plan, int32_t helper);
/* Wave roles (ABI 8): one wavefront per segment, a lane per skeleton.  A block is 64 skeletons
 * and K waves; the K roles of the sibling-segment schedule (lanes_per_skeleton, a power of two
 * 2..8; 8 only with two waves per SIMD) are the block's waves instead of K lanes of one wave, so
 * sibling segments run on separate waves that meet at a barrier per tree level, each wave reads
 * its segment's topology as wave-uniform values, and no lane repeats another lane's work (a
 * segment with fewer lanes than effectors is solved by one wave, effector by effector, in the
 * reference's order: ik_bone_segment_3d.cpp:210-240).  The whole solve state lives in device
 * memory (state placement 2).  1 on, 0 off, -1 (default) automatic: off until mbik_plan_autotune
 * has timed it.  constraint_mode plans have their own wave-roles kernel (2, 4 or 8 roles; a
 * multi-effector segment's effector reads split over its waves where their dirty chains are
 * disjoint).  Plans with stabilization passes and plans whose setup tables (or constraint_mode
 * node caches) need 64-bit indices run without it.  Results do not depend on it. */
int32_t mbik_plan_set_wave_roles(mbik_plan *plan, int32_t roles);
/* Status of a plan's earlier launches, for callers that poll instead of waiting for the next
 * call's return code (ABI 6): *status = MBIK_STATUS_HELPER_TIMEOUT when a helper-wave launch of
 * this plan that has completed timed out (see mbik_plan_set_helper_wave), else 0.  Reading
 * does not clear it. */
#define MBIK_STATUS_HELPER_TIMEOUT 1u
int32_t mbik_plan_status(const mbik_plan *plan, uint32_t *status);
/* Test hook (ABI 6): the helper wave stops before producing record drop_record of each block
 * (-1: never), and the handshake deadline is timeout_us microseconds (0: the default two
 * seconds) -- to exercise the timeout path above.  Not for production use. */
int32_t mbik_plan_debug_helper(mbik_plan *plan, int32_t drop_record, int32_t timeout_us);
/* How the solve addresses the per-skeleton setup tables (D, CF, CD).  0 (default): with
 * 32-bit offsets from a buffer resource when every table is below 4 GiB, else with 64-bit
 * element indices.  1: always 64-bit indices (state placement 0 only: placements 1 and 2 need
 * the 32-bit form and return MBIK_EUNSUPPORTED, which mbik_plan_autotune skips).  Plans whose
 * tables reach 4 GiB therefore solve in placement 0, and mbik_group_solve launches them on
 * their own.  Results do not depend on it. */
int32_t mbik_plan_set_table_addressing(mbik_plan *plan, int32_t wide);
/* Re-derives the per-skeleton setup data (bone-direction frames, Kusudama cones, tangent
 * circles and twist frames -- what mbik_plan_create computes on the host from the setup
 * pose, ManyBoneIK3D::_bone_list_changed many_bone_ik_3d.cpp:1011-1068) on the GPU for
 * skeletons [first, first+count), from device buffers indexed from skeleton `first`:
 * setup_pose [count][bones][10], cones [count][constraints][max_cones][4], twist
 * [count][constraints][2].  Same topology, pins and constraint bones as the plan; the
 * result equals the host builder's.  Synchronizes hip_stream. */
int32_t mbik_plan_rebuild_setup(mbik_plan *plan, int32_t first, int32_t count, const float *setup_pose,
		const float *cones, const float *twist, void *hip_stream);
/* GPU-side plan build for a crowd of distinct rigs: the segmentation, effector
 * lists, heading weights (generate_default_segments ik_bone_segment_3d.cpp:352-427,
 * update_pinned_list :74-88, create_headings_arrays / recursive_create_penalty_array
 * :281-343), damping, effector paths and constraint slots of every rig are built on `device`,
 * one GPU thread per rig (topo.h), and each rig's per-skeleton frames by mbik_setup_kernel
 * from device buffers: setup_pose[i] [n_skeletons[i]][bones][10], cones[i] / twist[i] as for
 * mbik_plan_rebuild_setup (NULL for rigs without constraints).  The host only reads the built
 * tables back to size the launch layout; the damping cosines cos(damp/2) come from the host's
 * libm (the reference's: the device's double cos differs in the last bit on ~1.6 % of inputs).
 * out_plans[i] receives rig i's plan (equal to what mbik_plan_create builds from the same
 * inputs); on error no plan is returned.  Combine them with mbik_group_create. */
int32_t mbik_plan_create_device(int32_t n_rigs, const mbik_skeleton_desc *descs, const mbik_config *configs,
		const int32_t *n_skeletons, const float *const *setup_pose, const float *const *cones, const float *const *twist,
		int32_t device, mbik_plan **out_plans);
/* mbik_plan_create_device with creation options, the same for every rig (ABI 4). */
int32_t mbik_plan_create_device_opts(int32_t n_rigs, const mbik_skeleton_desc *descs, const mbik_config *configs,
		const mbik_plan_options *opts, const int32_t *n_skeletons, const float *const *setup_pose, const float *const *cones,
		const float *const *twist, int32_t device, mbik_plan **out_plans);
/* Self-test of the GPU topology build: builds the n rigs with topo.h on `device` (or on the
 * host when device < 0: the same code) and compares every topology table with the host
 * builder's (mbik_plan_create's).  mismatches[i] = number of differing tables of rig i (0 when
 * equal, also when both refuse the rig with the same error); mbik_last_error() names the
 * first difference. */
int32_t mbik_selftest_topology(int32_t n_rigs, const mbik_skeleton_desc *descs, const mbik_config *configs, int32_t device,
		int32_t *mismatches);
/* Copies the plan's per-skeleton setup tables to host buffers (any may be NULL):
 * D [bones][9][n], CF [slots][14 + 31*max_cones][n] floats, CD [slots][2*max_cones][n]
 * doubles, n = skeleton_count; slots = constraints on bones in the IK bone list
 * (mbik_plan_info.constraint_slots; the strides are mbik_plan_info.cf_stride / cd_stride). */
int32_t mbik_plan_setup_tables(const mbik_plan *plan, float *D, float *CF, double *CD);
/* Diagnostic: how many one-wave blocks using lds_bytes_per_block of LDS one CU of the plan's
 * device holds at once (the runtime occupancy query for the plan's kernel). */
int32_t mbik_plan_resident_blocks(const mbik_plan *plan, int64_t lds_bytes_per_block);
/* Times candidate layouts on a real batch and keeps the fastest as the plan's layout: lanes
 * per skeleton (the widest sibling level or half of it), skeletons per block, checkpoint
 * interval, heading staging, state placement and waves per SIMD; dimensions pinned by the
 * setters above (a value other than 0 / -1) are kept.  A launch that is fully resident at the
 * default layout is left as it is (one skeleton's chain bounds it).  Runs the solve several
 * times from pose_in into pose_out (identical results); candidates within 1.5 % of the fastest
 * count as tied and the earliest in the candidate order wins, so that timing noise does not
 * change the pick from box to box; the two buffers must not overlap
 * (MBIK_EINVAL otherwise).  Synchronizes hip_stream.  The chosen layout is
 * fixed afterwards; mbik_plan_set_layout(plan, 0, 0, 0) and the staging / placement / waves
 * setters with -1 return to the defaults. */
int32_t mbik_plan_autotune(mbik_plan *plan, int32_t first, int32_t count, const float *pose_in, const float *targets,
		float *pose_out, void *hip_stream);

/* One frame for skeletons [first, first+count): device pointers (hipMalloc'd, on the
 * plan's device), asynchronous on hip_stream (NULL = default stream).  pose_in, targets
 * and pose_out are indexed from skeleton `first`; pose_out may equal pose_in (in place).
 *
 * Size limits (MBIK_EUNSUPPORTED, from mbik_plan_create or the first solve):
 *   - an effector's path from the root may hold at most MBIK_MAX_PATH_BONES bones;
 *   - the LDS of one launch block, mbik_plan_info.lds_bytes_per_block = the topology tables
 *     plus the solve state of its skeletons (state placement 0 keeps ~12 floats per bone and
 *     ~25 per pin per skeleton there, placement 2 none), must fit MBIK_MAX_LDS_BYTES; the
 *     automatic layout shrinks skeletons per block and moves state to device memory first,
 *     so only the topology tables of a very large rig (several thousand bones) hit this;
 *   - constraint_mode stages its per-lane stacks in LDS with the same limit;
 *   - mbik_pose_globals keeps one skeleton's poses and globals (22 floats per bone) in LDS with
 *     the same limit: a rig may have at most MBIK_FK_MAX_BONES bones there (the solve itself
 *     takes larger rigs);
 *   - mbik_skin_vertices keeps one skeleton's skin transforms (12 floats per bone) in LDS with the
 *     same limit: a mesh may be bound to at most MBIK_SKIN_MAX_BONES bones (mbik_mesh_create);
 *   - mbik_skin_vertices_shaped stages a skeleton's shape weights with its skin transforms:
 *     bone_count * 48 + shape_count * 4 bytes must fit the same limit (mbik_mesh_create_shaped). */
#define MBIK_MAX_PATH_BONES 4096
#define MBIK_MAX_LDS_BYTES (160 * 1024)
#define MBIK_FK_MAX_BONES 1861
#define MBIK_SKIN_MAX_BONES 3413
int32_t mbik_solve(mbik_plan *plan, int32_t first, int32_t count, const float *pose_in, const float *targets,
		float *pose_out, void *hip_stream);
/* mbik_solve plus a per-skeleton status byte (device buffer of `count` bytes, indexed from
 * skeleton `first`): nonfinite[i] = 1 when any bone of skeleton first+i ended the frame with
 * a non-finite basis, which is written out as the identity rotation exactly as
 * IKBone3D::set_skeleton_bone_pose does (ik_bone_3d.cpp:174-176); 0 otherwise.  The
 * reference reports nothing; the flag lets a caller find the skeletons it silently reset. */
int32_t mbik_solve_checked(mbik_plan *plan, int32_t first, int32_t count, const float *pose_in, const float *targets,
		float *pose_out, uint8_t *nonfinite, void *hip_stream);
/* Same with host buffers; synchronous (copies in, solves, copies out). */
int32_t mbik_solve_host(mbik_plan *plan, int32_t first, int32_t count, const float *pose_in, const float *targets,
		float *pose_out);
/* == IKEffector3D::update_target_global_transform for every pin of skeletons [first,
 * first+count) (ik_effector_3d.cpp:77-84, called by _update_ik_bones_transform,
 * many_bone_ik_3d.cpp:91-102): targets[s][e] = skeleton_global[s].affine_inverse() *
 * target_global[s][e] where visible[s][e] != 0 (visible NULL = every target node visible in
 * the tree); elsewhere targets[s][e] keeps its previous value, as the reference keeps
 * target_relative_to_skeleton_origin.  Transforms are 12 floats (basis rows, origin):
 * skeleton_global [count][12], target_global and targets [count][pins][12], visible
 * [count][pins] bytes; device pointers indexed from `first`, asynchronous on hip_stream. */
int32_t mbik_capture_targets(mbik_plan *plan, int32_t first, int32_t count, const float *skeleton_global,
		const float *target_global, const uint8_t *visible, float *targets, void *hip_stream);
/* The back half of a frame (ABI 9).  == Skeleton3D::get_bone_global_pose for every bone of `count`
 * skeletons (ik_bone_3d.cpp:71 is the reference's own call), and optionally the skin transform
 * global * bind_inverse and each pin's distance to its target.  Device buffers, asynchronous on
 * hip_stream (the plan's first call also uploads its bone schedule, synchronously):
 *   pose         [count][bones][10], e.g. mbik_solve's pose_out on the same stream
 *   inv_bind     [bones][12] per rig (basis rows, origin), or NULL
 *   globals      [count][bones][12] basis rows, then origin (the layout of `targets`), or NULL
 *   targets      [count][pins][12]; needed for pin_distance
 *   pin_distance [count][pins], or NULL
 * local(b) = Basis(rotation) * diag(scale) with origin = position (gd_math.h pose_to_xform);
 * global(b) = local(b) for a parentless bone, else global(parent) * local(b), for every bone of
 * the skeleton, also those outside the IK bone list; globals[s][b] = global(b) * inv_bind[b] when
 * inv_bind is given, else global(b); pin_distance[s][e] = |global(pins[e].bone).origin -
 * targets[s][e].origin|, always from the unskinned global.  Godot's operation order, unfused
 * (bitwise the reference's float results; mbik_pose_globals_cpu gives the same bits).
 * Only the rig (parents in any order, pin bones) is read from the plan, no per-skeleton table:
 * there is no `first`, and count may exceed the plan's skeleton count.  At least one of globals
 * and pin_distance must be non-NULL, pin_distance needs targets, and pose must not overlap
 * globals (MBIK_EINVAL).  count == 0 returns MBIK_OK without a launch; a plan without pins
 * ignores pin_distance; non-finite values propagate.  Buffers need float alignment only (16-byte
 * aligned ones move 16 bytes a lane).  Rigs above MBIK_FK_MAX_BONES bones: MBIK_EUNSUPPORTED. */
int32_t mbik_pose_globals(mbik_plan *plan, int32_t count, const float *pose, const float *inv_bind,
		float *globals, const float *targets, float *pin_distance, void *hip_stream);
/* Host-only (no device needed, like mbik_describe_topology): the same arithmetic from the same
 * code, host buffers, for a rig description (bone_count, parents, pins; any bone count). */
int32_t mbik_pose_globals_cpu(const mbik_skeleton_desc *desc, int32_t count, const float *pose,
		const float *inv_bind, float *globals, const float *targets, float *pin_distance);

/* Modifier influence (ABI 11): ManyBoneIK3D is a SkeletonModifier3D, and Godot 4.3's
 * Skeleton3D::_process_modifiers blends every bone's pose from before the modifier with the
 * modifier's by the inherited `influence` property.  mbik_solve is _process_modification alone;
 * this is that blend, on the device and on the stream of the solve, between mbik_solve and
 * mbik_pose_globals.  Device buffers, asynchronous on hip_stream:
 *   pose_in   [count][bones][10] the poses the modifier was given (mbik_solve's pose_in)
 *   pose_mod  [count][bones][10] the modifier's result (mbik_solve's pose_out)
 *   influence the weight of every skeleton, unless
 *   influence_per_skeleton [count] is given (device memory, read by the kernel, never by the host)
 *   pose_out  [count][bones][10]
 * Per bone, a = pose_in[s][b], m = pose_mod[s][b], w the skeleton's weight; float32, unfused:
 *   1. !(w < 1), i.e. w >= 1 or NaN: out = m, the same bits (Godot does not blend).
 *   2. A = Basis(a.rotation) * diag(a.scale) with origin a.position (Skeleton3D::get_bone_pose), M
 *      likewise; when all 12 floats compare equal (+0 == -0, NaN != NaN): out = m, the same bits
 *      (_process_modifiers' "avoid unneeded calculation"; q against -q takes this path).
 *   3. A negative w (not -0) counts as 0.  The one deviation: the property's range is 0..1 and
 *      Godot would extrapolate.
 *   4. Transform3D::interpolate_with: sa = A.basis.get_scale(), qa = A.basis.
 *      get_rotation_quaternion(), sm and qm from M; q = qa.slerp(qm, w).normalized()
 *      (Quaternion::slerp: a double sine over a float one for the start's coefficient),
 *      sc = sa.lerp(sm, w), o = A.origin.lerp(M.origin, w) (Vector3::lerp: a + (b - a) * w),
 *      T.basis.set_quaternion_scale(q, sc).
 *   5. Skeleton3D::set_bone_pose: out.rotation = T.basis.get_rotation_quaternion(), out.scale =
 *      T.basis.get_scale(), out.position = o.
 * w = 0 runs 4 and 5 like any weight: the result is the round-tripped input, as in Godot.
 * Non-finite values propagate; a NaN result of 4 and 5 is written as the quiet NaN 0x7fc00000.
 * mbik_pose_blend_cpu gives the same bits, and on finite poses the bits of that sequence on a
 * host with the plan's libm_variant.
 * Only the device, the bone count and libm_variant are read from the plan: there is no `first`,
 * count may exceed the plan's skeleton count, and every bone of the skeleton is blended.
 * pose_out may be exactly pose_mod or exactly pose_in (in place); any other overlap of pose_out
 * with an input, a null pose pointer or a negative count is MBIK_EINVAL.  count == 0 returns
 * MBIK_OK without a launch.  Buffers need float alignment only; element offsets are 64-bit. */
int32_t mbik_pose_blend(mbik_plan *plan, int32_t count, const float *pose_in, const float *pose_mod, float influence,
		const float *influence_per_skeleton, float *pose_out, void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, for any
 * bone count; libm_variant is MBIK_LIBM_VARIANT_* (MBIK_EINVAL otherwise). */
int32_t mbik_pose_blend_cpu(int32_t bone_count, int32_t libm_variant, int32_t count, const float *pose_in,
		const float *pose_mod, float influence, const float *influence_per_skeleton, float *pose_out);

/* Animation clip sampling (ABI 12): the front stage of a frame.  In Godot the poses a
 * SkeletonModifier3D receives were written by an animation; in a crowd each character plays its
 * own clip at its own time.  A clip set holds several clips for one rig, resident on one device,
 * shared by every skeleton; mbik_clip_sample writes mbik_solve's pose_in on the solve's stream from
 * one time and one clip index per skeleton (12 bytes a skeleton instead of 40 bytes a bone).
 *
 * A set is its own handle, bound to a bone count, a device and a libm_variant, not to a plan (as
 * mbik_mesh is).  mbik_clipset_create reads host arrays, checks them and uploads a repacked copy
 * synchronously; a set is immutable afterwards.  A track holds the keys of one channel of one
 * bone; a (bone, channel) without keys is untracked and samples to the rest pose.  MBIK_EINVAL: a
 * null `out`, rest_pose or clips; a negative count; clip_count == 0; an unknown libm_variant,
 * channel, interpolation or loop mode; a bone outside [0, bone_count); two tracks with keys for
 * the same (bone, channel) in one clip; a length that is not finite or not positive; key times
 * that are not strictly increasing, not finite or outside [0, length]; a null times or values with
 * key_count > 0.  The kernel relies on these checks and tests no key index itself.
 *
 * Semantics -- Godot 4.3's Animation::_interpolate for INTERPOLATION_NEAREST / INTERPOLATION_LINEAR,
 * LOOP_NONE / LOOP_LINEAR, forward playback, every key's transition 1.  Per skeleton s, t = time[s],
 * C = the clip clip_index[s] (or `clip` when clip_index is NULL):
 *   1. clip_index[s] outside [0, clip_count): every float of the skeleton is the quiet NaN
 *      0x7fc00000; no table is read.
 *   2. t not finite: every tracked channel is 0x7fc00000, no key is read; untracked channels as 4.
 *   3. t' (double): LOOP_NONE t' = t < 0 ? 0 : (t > length ? length : t); LOOP_LINEAR t' =
 *      fposmod(t, length): v = fmod(t, length); if (v < 0) v += length; v += 0.0.
 *   4. An untracked channel: the rest pose's bits for that bone and channel.
 *   5. A tracked channel with key times T[0..n-1], values V, wrap = (loop_mode linear && loop_wrap):
 *      i = the last key with T[i] <= t' (exact double compare), -1 if none.  n == 1: V[0].  Not
 *      wrap: i < 0 gives V[0], i == n-1 gives V[n-1], otherwise a = i, b = i+1, delta =
 *      (float)(T[b] - T[a]), from = (float)(t' - T[a]).  wrap: interior i as above; i == n-1: a = n-1,
 *      b = 0, delta = (float)((length - T[a]) + T[0]), from = (float)(t' - T[a]); i < 0: a = n-1,
 *      b = 0, end = length - T[a], delta = (float)(end + T[0]), from = (float)(end + t').  Sums and
 *      differences in double, rounded once.  c = |delta| < CMP_EPSILON (1e-5) ? 0 : from / delta
 *      (IEEE float division).  Nearest: V[a].  Linear position / scale: V[a] + (V[b] - V[a]) * c
 *      (Vector3::lerp), float32, unfused.  Linear rotation: Quaternion::slerp(V[a], V[b], c) as in
 *      mbik_pose_blend, not renormalised; key quaternions are used as given.
 *   6. A NaN produced by the arithmetic of 5 is stored as 0x7fc00000; copied bits stay as they are.
 * mbik_clip_sample_cpu gives the same bits from the same code.  Deviations from Godot: _find treats
 * a time within is_equal_approx of a key as that key, here the compare is exact; ping-pong,
 * backward playback and key transitions (ease) are not covered.  Cubic interpolation is taken by
 * sets made with mbik_clipset_create_desc, below (step 5c); this entry refuses it.
 * AnimationMixer's blend of several animations is mbik_clip_sample_layers, below (mbik_pose_blend is
 * the modifier's `influence`, a different function). */
typedef struct mbik_clip_track {
	int32_t bone;            /* [0, bone_count) */
	int32_t channel;         /* 0 position (3 floats a key), 1 rotation (4: x,y,z,w), 2 scale (3) */
	int32_t interpolation;   /* 0 nearest, 1 linear; 2 cubic through mbik_clipset_desc only */
	int32_t loop_wrap;       /* Animation track loop_wrap */
	int32_t key_count;       /* 0 allowed: same as no track */
	const double *times;     /* [key_count] seconds, strictly increasing, finite, in [0, length] */
	const float *values;     /* [key_count][3 or 4] */
} mbik_clip_track;
typedef struct mbik_clip_desc {
	double length;           /* > 0, finite */
	int32_t loop_mode;       /* 0 none, 1 linear */
	int32_t track_count;
	const mbik_clip_track *tracks;
} mbik_clip_desc;
typedef struct mbik_clipset mbik_clipset;
int32_t mbik_clipset_create(int32_t bone_count, const float *rest_pose /* [bones][10] */, int32_t clip_count,
		const mbik_clip_desc *clips, int32_t libm_variant, int32_t device, mbik_clipset **out);
void mbik_clipset_destroy(mbik_clipset *set);
/* Samples the set for `count` skeletons into pose_out [count][bones][10], the layout mbik_solve
 * reads.  Device buffers on the set's device, asynchronous on hip_stream (NULL = default stream);
 * time and clip_index are read by the kernel only, never by the host.  count == 0 or a set without
 * bones returns MBIK_OK without a launch.  MBIK_EINVAL: a null time or pose_out, a negative count,
 * or (with clip_index NULL) a `clip` outside the set.  Buffers need natural alignment only (float
 * for pose_out, 8 bytes for time); element offsets are 64-bit. */
int32_t mbik_clip_sample(mbik_clipset *set, int32_t count, const double *time /* device [count] */,
		const int32_t *clip_index /* device [count], or NULL */, int32_t clip /* used when clip_index is NULL */,
		float *pose_out /* device [count][bones][10] */, void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with
 * mbik_clipset_create's and mbik_clip_sample's checks. */
int32_t mbik_clip_sample_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *pose_out);

/* Layered clip sampling: AnimationMixer's blend of several animations, in one call and one kernel.
 * Characters of a crowd cross-fade walk into run and carry partial-weight layers; each skeleton
 * has layer_count records (time, clip, weight), and the call writes the blend of their samples.
 * Purely additive to ABI 15: two new symbols and one new struct, no existing struct or call
 * changed, MBIK_ABI_VERSION stays 15.  A caller detects the feature by the presence of the symbol
 * mbik_clip_sample_layers (dlsym, or MBIK_CLIP_MAX_LAYERS at compile time).
 *
 * Semantics -- Godot's core is not part of the reference tree, so mbik_clip_sample_layers_cpu is
 * the specification, modelled on Godot 4.3's AnimationMixer::_blend_init / _blend_calc_total_weight
 * / _blend_process / _blend_apply: every layer's offset from the rest pose is accumulated,
 * loc += (x - init) * blend and rot = (rot * slerp(identity, init^-1 * x, blend)).normalized().
 * Without MBIK_CLIP_LAYERS_NORMALIZE the mode is the mixer's deterministic one (blend = weight);
 * with it the non-deterministic one, which is AnimationPlayer's cross-fade (blend = weight / the
 * channel's total weight).  All arithmetic is float32 and unfused, in the order written.  For
 * skeleton s, bone b and channel ch (position, rotation, scale), I = the rest pose's value of that
 * channel (init_loc / init_rot / init_scale), K = layer_count:
 *   1. For l = 0 .. K-1: a layer with clip == -1 is off -- nothing of it is read, its time and
 *      weight may be anything.  Any other clip outside [0, clip_count) makes the whole skeleton
 *      invalid: every float of it is 0x7fc00000 and no table is read (mbik_clip_sample's step 1).
 *      The kernel makes this test itself, before any table access.
 *   2. w = weight; if (w < 0) w = 0; if (w > 1) w = 1.  A NaN passes both compares and propagates.
 *   3. A layer that is on contributes to (b, ch) when its clip tracks that channel (at least one
 *      key).  Other layers do not exist for that channel.
 *   4. Without the flag blend_l = w_l.  With it: total = 0.0f, total = total + w_l over the
 *      contributing layers, ascending; |total| < CMP_EPSILON (1e-5): the channel receives nothing
 *      (step 6); otherwise blend_l = w_l / total (IEEE float division).
 *   5. acc = I.  For each contributing layer, ascending: |blend_l| < CMP_EPSILON (false for NaN):
 *      the layer is skipped and none of its keys is read (Godot's is_zero_approx(blend)).
 *      Otherwise x = the channel's value exactly as mbik_clip_sample's steps 2 to 6 give it for
 *      (time_l, clip_l), 0x7fc00000 for a non-finite time included, and
 *        position, scale:  acc = acc + (x - I) * blend_l   (V3 - V3, V3 * float, V3 + V3)
 *        rotation:         d = inverse(I) * x  (conjugate; Quaternion::operator*),
 *                          e = slerp(identity, d, blend_l)  (Quaternion::slerp as in mbik_pose_blend),
 *                          acc = normalized(acc * e).
 *   6. A channel that had at least one layer accumulated stores acc, any NaN as 0x7fc00000.  Every
 *      other channel -- untracked, all layers off or skipped, a zero total -- stores the rest
 *      pose's bits, copied.
 * Consequences: with K = 1 and w = 1 the result is I + (x - I) * 1 and normalized(I * (I^-1 * x)),
 * Godot's behaviour; it is not the bits of mbik_clip_sample.  Quaternions are used as given:
 * neither the rest pose nor the keys are renormalised on input.
 * Deviations from Godot: step 2's clamp (Godot would extrapolate; the slerp's double sine needs its
 * argument in [0, pi/2], the reason mbik_pose_blend gives for clamping negative weights; additive
 * layers are out of scope).  init_* are the rest pose's ten floats as given (Godot derives them
 * from the rest Transform3D).  Per-track blend weights (filters), RESET animations and
 * post_process_key_value are not covered.  Root motion is mbik_clip_root_motion_layers, below.
 *
 * MBIK_EINVAL: a null set; count < 0; layer_count outside [1, MBIK_CLIP_MAX_LAYERS]; unknown flag
 * bits; and, when there is work to do, a null layers or pose_out, layers not 8-byte aligned, or
 * pose_out overlapping layers.  count == 0 or a set without bones returns MBIK_OK without a launch.
 * Device buffers on the set's device, asynchronous on hip_stream; layers is read by the kernel
 * only, never by the host.  layers needs 8-byte alignment (a 16-byte aligned array moves one load
 * a record), pose_out float alignment; element offsets are 64-bit; mbik_clip_sample's limit of
 * 2^39 bones a call applies. */
typedef struct mbik_clip_layer {
	double time;             /* seconds, as mbik_clip_sample's time[s] */
	int32_t clip;            /* [0, clip_count), or -1: the layer is off */
	float weight;            /* clamped into [0, 1] */
} mbik_clip_layer;           /* 16 bytes */
#define MBIK_CLIP_MAX_LAYERS 8
#define MBIK_CLIP_LAYERS_NORMALIZE 1u
int32_t mbik_clip_sample_layers(mbik_clipset *set, int32_t count, int32_t layer_count,
		const mbik_clip_layer *layers /* device [count][layer_count] */, uint32_t flags,
		float *pose_out /* device [count][bones][10] */, void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with
 * mbik_clipset_create's and mbik_clip_sample_layers' checks. */
int32_t mbik_clip_sample_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags, float *pose_out);

/* Root motion: AnimationMixer's root_motion_track for a crowd.  Three stages of a frame take
 * skeleton_global [count][12], each character's world transform; these calls produce it on the
 * device.  Per skeleton, the extraction calls write the root bone's motion over the frame -- from
 * the previous time to the time of each layer, with the loop seam handled -- into a motion record,
 * hold the root bone at rest in the pose, and mbik_root_motion_apply composes the record into
 * skeleton_global in place.  Purely additive to ABI 15: new symbols and one new flag, no existing
 * struct or call changed, the sample calls keep their bits, MBIK_ABI_VERSION stays 15.  A caller
 * detects the feature by the presence of the symbol mbik_clip_root_motion.
 *
 * A motion record is 10 floats in the pose record's order: the rotation delta x, y, z, w (what
 * AnimationMixer::get_root_motion_rotation returns), the position delta
 * (get_root_motion_position) and the scale delta (get_root_motion_scale).
 *
 * Semantics -- Godot's core is not part of the reference tree, so the _cpu entries are the
 * specification, modelled on the root_motion branches of the position, rotation and scale cases of
 * Godot 4.3's AnimationMixer::_blend_process.  mbik_clip_root_motion is defined as
 * mbik_clip_root_motion_layers with one record (time[s], clip_index[s] or clip, 1.0f),
 * time_prev[s] and flags 0; it is one code path and gives the same bits.  All arithmetic is
 * float32 and unfused, in the order written.  For skeleton s, root bone r and each channel ch of
 * r, K = layer_count:
 *   1. Validity is mbik_clip_sample_layers' step 1: a layer with clip == -1 is off -- nothing of
 *      it is used, its time_prev included.  Any other clip outside [0, clip_count) makes all 10
 *      floats of the record 0x7fc00000; that is decided from the records before any table access,
 *      and pose[s] is then left untouched.
 *   2. w_l, the contributing layers, the channel's total and blend_l are exactly what
 *      mbik_clip_sample_layers' steps 2 to 5 compute for bone r.  A layer is skipped without
 *      reading a key when its clip does not track the channel or |blend_l| < CMP_EPSILON.
 *   3. The segments of layer l, with t1 = layers[l].time, t0 = time_prev[l], L = the clip's length.
 *      Both finite: p0 = t0 and p1 = t1 mapped by mbik_clip_sample's step 3; looped = (loop_mode
 *      linear && p0 > p1), an exact double compare.  Not looped: one segment (p0, p1).  Looped:
 *      two segments in this order, (p0, L) then (+0.0, p1).  Either time not finite: one segment
 *      whose two values are both 0x7fc00000, and no key is read.
 *   4. X(u) is the channel's value at the already mapped time u by mbik_clip_sample's steps 5 and
 *      6; there is no second time mapping, so X(L) on a looping clip is the value at the end of
 *      the clip, not the value at fposmod's 0.
 *   5. Accumulation over the contributing layers, ascending, and each layer's segments (u0, u1) in
 *      order, from position +0,+0,+0, scale +0,+0,+0 and rotation 0,0,0,1:
 *        position, scale:  acc = acc + (X(u1) - X(u0)) * blend_l
 *        rotation:         acc = normalized(acc * slerp(identity, inverse(X(u0)) * X(u1), blend_l))
 *      with mbik_clip_sample_layers' slerp, inverse, quaternion product and normalized.
 *   6. A channel that accumulated at least one segment stores acc, any NaN as 0x7fc00000; every
 *      other channel stores its start value's bits.
 *   7. With pose non-NULL, pose[s][r][0..9] of every valid skeleton is overwritten with the rest
 *      pose's bits of bone r: Godot does not apply a root-motion track to the bone.  The call runs
 *      behind the sample call that wrote pose, on the same stream.
 * Deviations from Godot: forward playback only.  At most one wrap a frame is seen, as in Godot: a
 * frame longer than the clip loses whole loops.  On a LOOP_NONE clip p0 > p1 is a plain negative
 * difference.
 *
 * mbik_root_motion_apply, per skeleton: G = skeleton_global[s], basis rows then origin as in
 * mbik_capture_targets; q = the record's rotation, p = its position; the scale delta is not
 * applied.  G' = G * Transform3D(Basis(q), p) as Transform3D::operator*= computes it: origin' =
 * G.xform(p), basis' = G.basis * Basis(q) (Basis::set_quaternion, Basis::operator*).  With
 * MBIK_ROOT_MOTION_ORTHONORMALIZE basis' = basis'.orthonormalized(): a long walk otherwise drifts
 * off orthonormal.  Any NaN is stored as 0x7fc00000; non-finite input propagates.  The set names
 * the device only.
 *
 * MBIK_EINVAL: a null set; count < 0; root_bone outside [0, bone_count), so a set without bones is
 * always invalid here; layer_count outside [1, MBIK_CLIP_MAX_LAYERS]; unknown flag bits; a plain
 * `clip` outside the set when clip_index is NULL; and, when count > 0, a null required buffer
 * (pose and clip_index may be NULL), layers, time or time_prev not 8-byte aligned, motion_out
 * overlapping any input or pose, skeleton_global overlapping motion.  count == 0 returns MBIK_OK
 * without a launch.  Device buffers on the set's device, asynchronous on hip_stream; layers, the
 * times and clip_index are read by the kernel only, which tests every clip index before any table
 * access.  motion_out, pose and skeleton_global need float alignment. */
#define MBIK_ROOT_MOTION_ORTHONORMALIZE 1u
int32_t mbik_clip_root_motion(mbik_clipset *set, int32_t count, int32_t root_bone,
		const double *time_prev /* device [count] */, const double *time /* device [count] */,
		const int32_t *clip_index /* device [count], or NULL */, int32_t clip,
		float *motion_out /* device [count][10] */, float *pose /* device [count][bones][10], or NULL */, void *hip_stream);
int32_t mbik_clip_root_motion_layers(mbik_clipset *set, int32_t count, int32_t layer_count, int32_t root_bone,
		const mbik_clip_layer *layers /* device [count][layer_count], this frame's records */,
		const double *time_prev /* device [count][layer_count] */, uint32_t flags /* MBIK_CLIP_LAYERS_NORMALIZE */,
		float *motion_out, float *pose, void *hip_stream);
int32_t mbik_root_motion_apply(mbik_clipset *set, int32_t count, const float *motion /* device [count][10] */,
		uint32_t flags, float *skeleton_global /* device [count][12], in place */, void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with
 * mbik_clipset_create's checks and the checks above. */
int32_t mbik_clip_root_motion_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t root_bone, const double *time_prev, const double *time,
		const int32_t *clip_index, int32_t clip, float *motion_out, float *pose);
int32_t mbik_clip_root_motion_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t layer_count, int32_t root_bone, const mbik_clip_layer *layers,
		const double *time_prev, uint32_t flags, float *motion_out, float *pose);
int32_t mbik_root_motion_apply_cpu(int32_t count, const float *motion, uint32_t flags, float *skeleton_global);

/* Playback: AnimationPlayer for a crowd.  The layered calls above read layers [count][K] and
 * time_prev [count][K]; a playback object keeps what produces them -- per skeleton the current
 * animation's position and speed, the clips of a cross-fade that are still fading out, whether
 * the clip has ended -- on the device, and mbik_playback_advance moves it one frame on and writes
 * both arrays there.  A playing crowd then uploads its events only (somebody starts a new clip):
 * a list of commands, and nothing at all on a frame without one.  It is AnimationPlayer's play()
 * with a blend time, speed_scale, animation_set_next and set_blend_time.  Purely additive to ABI
 * 15: new symbols and structs only, no existing struct or call changed, MBIK_ABI_VERSION stays 15.
 * A caller detects the feature by the presence of the symbol mbik_playback_advance.
 *
 * A playback object owns the state of `capacity` skeletons with K = layer_count slots each, on
 * the set's device.  It takes the clip count and each clip's length and loop_mode from the set
 * when it is created; the set may be destroyed before the object.  A new object has every slot
 * off.  mbik_playback_write and mbik_playback_read convert skeletons [first, first + n) from and
 * to the public records (host memory, [n][K] slots and [n] flag words); they are synchronous, and
 * the caller orders them against advances in flight on other streams.
 *
 * State of one skeleton.  Slot 0 is the current animation (its blend_left and blend_time are
 * stored as +0).  Slots 1..K-1 are the clips fading out, oldest first and compact: an off slot
 * (clip == -1, every other field +0) is followed only by off slots, slot 0 included.  Its flag
 * word holds MBIK_PLAYBACK_STARTED (slot 0 was started and has not been shown yet) and
 * MBIK_PLAYBACK_ENDED (slot 0's LOOP_NONE clip has run to its end).
 *
 * Semantics -- Godot's core is not part of the reference tree, so mbik_playback_advance_cpu is the
 * specification, modelled on Godot 4.3's AnimationPlayer::play, _process_playback_data and
 * _blend_playback_data.  The device runs the same code and gives the same bits.  Every operation
 * is IEEE and unfused, in the order written; "time mapping" is mbik_clip_sample's step 3 (clamp
 * into [0, L] for LOOP_NONE, fposmod for LOOP_LINEAR); L and loop_mode are those of the slot's
 * clip; max(0, x) is (x > 0 ? x : +0).  For skeleton s < count, in this order:
 *   A. Commands.  The list is sorted by skeleton, non-decreasing.  lo = 0, hi = cmd_count; while
 *      lo < hi: mid = lo + (hi - lo) / 2; cmds[mid].skeleton < s ? lo = mid + 1 : hi = mid.  Then
 *      the entries i = lo, lo + 1, ... are applied in order while i < cmd_count and
 *      cmds[i].skeleton == s.  An unsorted list gives whatever that search gives; nothing outside
 *      [0, cmd_count) is read, and an entry whose skeleton lies outside [0, count) is never
 *      applied.  One command:
 *        clip == -1: stop -- every slot off, flags 0.
 *        clip outside [-1, clip_count), or speed not finite: ignored, event BAD_COMMAND.
 *        otherwise play(clip, start, speed, blend_time):
 *          bt = blend_time if blend_time >= 0; else (negative or NaN) blend_times[from][clip]
 *          with from = slot 0's clip, when slot 0 is on and the table was given; else
 *          default_blend_time (0 without a desc).
 *          If slot 0 is on and bt > 0: cur = max(0, 1.0f - sum) with sum the float sum of the
 *          fades' blend_left from +0, ascending; the fade (slot 0's clip, pos, speed, blend_left
 *          = cur, blend_time = bt) is appended behind the last fade.  Without a free slot the
 *          oldest fade (slot 1) is dropped first and the others move up, event FADE_DROPPED; with
 *          K == 1 the new fade itself is dropped, with the same event.  Otherwise (slot 0 off, or
 *          not bt > 0) every fade goes off.
 *          Slot 0 becomes (clip, start', speed, +0, +0) and flags become STARTED.  start' is the
 *          time mapping of a finite start; of any other start, L when speed's sign bit is set,
 *          else +0.0.
 *   B. Advance.  g = (double)speed_scale * delta.  An on slot has step = g * (double)speed and
 *      prev = pos.  "pos advances" means n = pos + step and, if n is finite, pos = the time
 *      mapping of n (else pos stays).
 *      Slot 0, when on: with STARTED the bit is cleared, event STARTED, pos stays -- the first
 *      frame of a clip shows its start, as Godot's p_started does.  Else with ENDED pos stays.
 *      Else pos advances; then for LOOP_NONE, (step > 0 && n >= L) || (step < 0 && n <= 0) sets
 *      ENDED, raises event ENDED and takes every fade off (AnimationPlayer clears its blend list
 *      at end_reached); for LOOP_LINEAR, pos != n raises event LOOPED.
 *      Each fade j >= 1 that is still on: pos advances (no flags, no events), and blend_left =
 *      blend_left - (float)(fabs(g) / (double)blend_time).  A fade with !(blend_left > 0) goes
 *      off.  Then the fades are compacted, stably.
 *   C. Output.  layers_out[s][j] = (pos_j, clip_j, w_j) and time_prev_out[s][j] = prev_j, with
 *      w_j = blend_left_j for a fade and w_0 = max(0, 1.0f - sum) over the fades that are left,
 *      summed as in A.  An off slot writes (+0.0, -1, +0.0f) and +0.0.  These are the records
 *      mbik_clip_sample_layers, mbik_clip_sample_shapes_layers and mbik_clip_root_motion_layers
 *      take with MBIK_CLIP_LAYERS_NORMALIZE, AnimationPlayer's cross-fade.  Positions are already
 *      mapped, so root motion's p0 > p1 seam test works on them.  A skeleton whose slot 0 is off
 *      has every layer off and samples to the rest pose.
 *   D. Transition.  If ENDED was set in this advance and next was given and next[slot 0's clip]
 *      >= 0: A's play(next, a NaN start, slot 0's speed, blend_time -1), event TRANSITIONED.  The
 *      next advance shows the new clip's start with time_prev == time; the clip that ended fades
 *      out from its end.
 *      events_out[s], when given, holds the events of A to D: STARTED, ENDED, LOOPED,
 *      TRANSITIONED, BAD_COMMAND, FADE_DROPPED.
 * Deviations from Godot: exact compares where Godot uses is_equal_approx / is_zero_approx; a fade
 * that has run down is removed at once (Godot keeps it one more frame at CMP_EPSILON); at most
 * K - 1 fades; no ping-pong; a command always restarts its clip, also the one that is playing; no
 * method, audio or signal side effects.  Backward playback (a negative speed or speed_scale)
 * advances and samples correctly; mbik_clip_root_motion* remain forward-only.  A command's
 * infinite blend_time is taken as it is: that fade never runs down, and mbik_playback_write
 * refuses such a record.
 *
 * MBIK_EINVAL: a null object, set, out or required buffer (events_out may be NULL; cmds may be
 * NULL when cmd_count is 0); capacity < 0; count outside [0, capacity]; layer_count outside
 * [1, MBIK_CLIP_MAX_LAYERS]; a desc whose struct_size is too small, with a next entry outside
 * [-1, clip_count), or with a blend time (default_blend_time included) that is not finite or
 * negative; delta or speed_scale not finite; cmd_count < 0; when count > 0, layers_out,
 * time_prev_out or cmds not 8-byte aligned, or outputs overlapping each other or cmds.  In
 * mbik_playback_write (and for the state given to the _cpu entry): a range outside the capacity;
 * unknown flag bits; a clip outside [-1, clip_count); on an on slot a pos that is not finite or
 * outside [0, L], or a speed that is not finite; an on fade without a finite blend_time > 0 and a
 * finite blend_left; an on slot behind an off slot.  write stores slot 0's fade fields and every
 * field of an off slot as +0.  count == 0 returns MBIK_OK without a launch.  Device buffers on
 * the set's device, asynchronous on hip_stream; the commands are read by the kernel only, which
 * tests every field before it uses it; events_out needs no alignment. */
typedef struct mbik_playback_slot {
	double pos;              /* seconds into the clip, in [0, length] */
	int32_t clip;            /* [0, clip_count), or -1: the slot is off */
	float speed;             /* the slot's own speed; negative plays backward */
	float blend_left;        /* a fade's weight; runs down to 0 over blend_time */
	float blend_time;        /* seconds */
} mbik_playback_slot;        /* 24 bytes */
typedef struct mbik_playback_cmd {
	double start;            /* seconds; not finite: the clip's start (its end for a speed with the sign bit set) */
	int32_t skeleton;
	int32_t clip;            /* [0, clip_count): play; -1: stop */
	float blend_time;        /* seconds; negative or NaN: the desc's */
	float speed;
} mbik_playback_cmd;         /* 24 bytes */
typedef struct mbik_playback_desc {
	int32_t struct_size;     /* sizeof(mbik_playback_desc) */
	float default_blend_time;
	const int32_t *next;     /* [clip_count], -1 none (animation_set_next); or NULL */
	const float *blend_times; /* [clip_count][clip_count] from, to (set_blend_time); or NULL */
} mbik_playback_desc;
typedef struct mbik_playback mbik_playback;
#define MBIK_PLAYBACK_STARTED 1u      /* flag and event */
#define MBIK_PLAYBACK_ENDED 2u        /* flag and event */
#define MBIK_PLAYBACK_LOOPED 4u       /* events only, from here on */
#define MBIK_PLAYBACK_TRANSITIONED 8u
#define MBIK_PLAYBACK_BAD_COMMAND 16u
#define MBIK_PLAYBACK_FADE_DROPPED 32u
int32_t mbik_playback_create(mbik_clipset *set, int32_t capacity, int32_t layer_count, const mbik_playback_desc *desc /* or NULL */,
		mbik_playback **out);
void mbik_playback_destroy(mbik_playback *pb);
int32_t mbik_playback_write(mbik_playback *pb, int32_t first, int32_t n, const mbik_playback_slot *slots /* host [n][K] */,
		const uint32_t *flags /* host [n] */);
int32_t mbik_playback_read(mbik_playback *pb, int32_t first, int32_t n, mbik_playback_slot *slots, uint32_t *flags);
int32_t mbik_playback_advance(mbik_playback *pb, int32_t count, double delta, float speed_scale,
		const mbik_playback_cmd *cmds /* device [cmd_count], or NULL when 0 */, int32_t cmd_count,
		mbik_clip_layer *layers_out /* device [count][K] */, double *time_prev_out /* device [count][K] */,
		uint8_t *events_out /* device [count], or NULL */, void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with the
 * checks above; of a clip only length and loop_mode are looked at.  slots and flags are the state,
 * changed in place. */
int32_t mbik_playback_advance_cpu(int32_t clip_count, const mbik_clip_desc *clips, const mbik_playback_desc *desc /* or NULL */,
		int32_t count, int32_t layer_count, mbik_playback_slot *slots /* [count][K] */, uint32_t *flags /* [count] */, double delta,
		float speed_scale, const mbik_playback_cmd *cmds, int32_t cmd_count, mbik_clip_layer *layers_out, double *time_prev_out,
		uint8_t *events_out);

/* Blend-shape tracks of a clip set: the [count][shape_count] weights mbik_skin_vertices_shaped and
 * mbik_skin_vertices_call read, written on the device from the times, clip indices and layer
 * records that already drive the bones.  In Godot the same Animation resource carries
 * TYPE_BLEND_SHAPE tracks beside its position / rotation / scale tracks, AnimationMixer blends
 * them in the same pass and MeshInstance3D.set_blend_shape_value receives the result; here a
 * shaped set carries them beside its mbik_clip_desc array (as mbik_mesh_create_shaped carries
 * shapes beside a mesh), and two calls write the weights.  Purely additive to ABI 15: new symbols
 * and new structs only, MBIK_ABI_VERSION stays 15; a caller detects the feature by the symbol
 * mbik_clip_sample_shapes.
 *
 * mbik_clipset_create_shaped makes mbik_clipset_create's checks on its first arguments and builds
 * the same set: mbik_clip_sample and mbik_clip_sample_layers on it give the bits they give on a
 * set made by mbik_clipset_create.  bone_count == 0 (a face-only rig) is valid.  shapes->clips is
 * parallel to `clips`: entry c holds the shape tracks of clip c, which shares that clip's length
 * and loop_mode.  A shape without keys in a clip is untracked there.  Additional MBIK_EINVAL: a
 * null shapes; struct_size < sizeof(mbik_clipset_shapes); shape_count < 1; a null shapes->clips; a
 * negative track_count or a null tracks with tracks; a shape outside [0, shape_count); two tracks
 * with keys for the same shape in one clip; an unknown interpolation; a negative key_count; key
 * times that are not strictly increasing, not finite or outside [0, length]; a null times or
 * values with key_count > 0.  Key values and init are taken as given, non-finite ones included.
 *
 * Semantics -- the _cpu entries are the specification, modelled on Godot 4.3's
 * Animation::blend_shape_track_interpolate and the TYPE_BLEND_SHAPE case of
 * AnimationMixer::_blend_process.  P = shape_count, I_j = init[j] (+0 for a NULL init).
 * mbik_clip_sample_shapes, for skeleton s and shape j, is mbik_clip_sample's steps 1 to 6 with
 * "shape" for "(bone, channel)" and I_j's bits for the rest pose:
 *   1. clip_index[s] outside [0, clip_count): all P weights of the skeleton are 0x7fc00000; no
 *      table is read.
 *   2. t not finite: a tracked shape is 0x7fc00000, no key is read; an untracked shape as 4.
 *   3. t' exactly as mbik_clip_sample's step 3.
 *   4. An untracked shape: I_j's bits.
 *   5. A tracked shape: the key i, the keys a and b, delta, from and c exactly as mbik_clip_sample's
 *      step 5.  Nearest, or a pick without a second key: V[a]'s bits.  Linear:
 *      V[a] + (V[b] - V[a]) * c (Math::lerp), float32, unfused.
 *   6. A NaN produced by the arithmetic of 5 is stored as 0x7fc00000; copied bits stay as they are.
 * mbik_clip_sample_shapes_layers is mbik_clip_sample_layers' steps 1 to 6 with I = I_j and the
 * position / scale rule: a layer with clip == -1 is off; any other clip outside the set makes all
 * P weights of the skeleton 0x7fc00000, decided by the kernel before any table access, and for any
 * record array the verdict is the one mbik_clip_sample_layers gives; w is clamped into [0, 1]
 * (a NaN passes); a layer contributes to shape j when its clip has keys for j; blend_l = w_l, or
 * with MBIK_CLIP_LAYERS_NORMALIZE w_l / total over the contributing layers, a |total| <
 * CMP_EPSILON giving the shape nothing; acc = I_j, and per contributing layer, ascending, unless
 * |blend_l| < CMP_EPSILON (the layer is skipped, none of its keys read):
 *        acc = acc + (x - I_j) * blend_l,   x = the shape's value by steps 2 to 6 above;
 * a shape that had a layer accumulated stores acc, a NaN as 0x7fc00000; every other shape stores
 * I_j's bits.  With K = 1 and w = 1 the result is I + (x - I) * 1, not the bits of the plain call.
 * Not covered, as for the poses: cubic interpolation, ping-pong, backward playback, key
 * transitions (ease), per-track filters, additive layers.
 *
 * The sample calls: device buffers on the set's device, asynchronous on hip_stream; time,
 * clip_index and layers are read by the kernel only, never by the host.  MBIK_EINVAL: a null set; a
 * set without shapes; then mbik_clip_sample's / mbik_clip_sample_layers' checks with weights_out
 * for pose_out, and weights_out overlapping time, clip_index or layers.  count == 0 returns
 * MBIK_OK without a launch.  weights_out needs float alignment only (time 8 bytes, layers 8
 * bytes); element offsets are 64-bit; more than 2^39 weights a call is MBIK_EUNSUPPORTED. */
typedef struct mbik_shape_track {
	int32_t shape;           /* [0, shape_count) */
	int32_t interpolation;   /* 0 nearest, 1 linear */
	int32_t loop_wrap;       /* Animation track loop_wrap */
	int32_t key_count;       /* 0 allowed: same as no track */
	const double *times;     /* [key_count], mbik_clip_track's rules against the clip's length */
	const float *values;     /* [key_count] */
} mbik_shape_track;
typedef struct mbik_clip_shape_tracks {
	int32_t track_count;
	const mbik_shape_track *tracks;
} mbik_clip_shape_tracks;
typedef struct mbik_clipset_shapes {
	int32_t struct_size;     /* sizeof(mbik_clipset_shapes) */
	int32_t shape_count;     /* P >= 1 */
	const float *init;       /* [P], the RESET value of each shape; NULL: all +0 */
	const mbik_clip_shape_tracks *clips; /* [clip_count], parallel to the mbik_clip_desc array */
} mbik_clipset_shapes;
int32_t mbik_clipset_create_shaped(int32_t bone_count, const float *rest_pose /* [bones][10] */, int32_t clip_count,
		const mbik_clip_desc *clips, const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t device, mbik_clipset **out);
int32_t mbik_clip_sample_shapes(mbik_clipset *set, int32_t count, const double *time /* device [count] */,
		const int32_t *clip_index /* device [count], or NULL */, int32_t clip /* used when clip_index is NULL */,
		float *weights_out /* device [count][P] */, void *hip_stream);
int32_t mbik_clip_sample_shapes_layers(mbik_clipset *set, int32_t count, int32_t layer_count,
		const mbik_clip_layer *layers /* device [count][layer_count] */, uint32_t flags, float *weights_out /* device [count][P] */,
		void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with
 * mbik_clipset_create_shaped's and the sample calls' checks. */
int32_t mbik_clip_sample_shapes_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t count, const double *time, const int32_t *clip_index,
		int32_t clip, float *weights_out);
int32_t mbik_clip_sample_shapes_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t count, int32_t layer_count, const mbik_clip_layer *layers,
		uint32_t flags, float *weights_out);

/* Cubic interpolation: Godot's INTERPOLATION_CUBIC (interpolation == 2) on pose tracks and shape
 * tracks, through every call that reads a clip set.  Purely additive to ABI 15: three new symbols
 * and two new structs, no existing struct, call, table layout or result bit changed,
 * MBIK_ABI_VERSION stays 15.  A caller detects the feature by the presence of the symbol
 * mbik_clipset_create_desc.  The older creation entries and every older _cpu entry keep refusing
 * interpolation 2 as they did.
 *
 * mbik_clipset_create_desc is mbik_clipset_create (shapes NULL) or mbik_clipset_create_shaped, with
 * the same checks in the same order and the same messages, except that interpolation 2 is taken.
 * Every other value -- Godot's INTERPOLATION_LINEAR_ANGLE 3 and INTERPOLATION_CUBIC_ANGLE 4 among
 * them -- stays MBIK_EINVAL "unknown interpolation N", and loop_mode 2 (ping-pong) stays
 * MBIK_EINVAL.  MBIK_EINVAL before those checks: a null desc, a struct_size below
 * sizeof(mbik_clipset_desc), flags other than 0.  The device entries -- mbik_clip_sample, _layers,
 * _shapes, _shapes_layers, mbik_clip_root_motion, _layers, mbik_playback_create -- take such a set
 * unchanged.  A set without a cubic track, however it was made, runs the same kernels and gives the
 * same bits as before.
 *
 * mbik_clip_call_cpu is the one host-only twin of the six sampling and extraction calls on a set
 * described by a mbik_clipset_desc, which may hold cubic tracks.  kind selects the call; the fields
 * it does not name in its older _cpu entry are ignored.  Each kind makes the set's checks (as
 * mbik_clipset_create_desc; shapes are checked when given, and required by the two SHAPES kinds),
 * then the call checks of its older _cpu entry with the same messages in the same order, then runs
 * the same per-item code.  MBIK_EINVAL before those: a null set or call, a struct_size below the
 * struct's size, set flags other than 0, an unknown kind.
 *
 * Semantics -- Godot's core is not part of the reference tree, so mbik_clip_call_cpu is the
 * specification, modelled on Godot 4.3's Animation::_interpolate, Math::cubic_interpolate_in_time
 * and Quaternion::spherical_cubic_interpolate_in_time.  mbik_clip_sample's step 5, continued for a
 * cubic channel: all arithmetic float32 and unfused, in the order written; sums and differences of
 * times in double, rounded once to float; divisions IEEE; lerp(a, b, w) = a + (b - a) * w.
 *   5c. i, wrap as in step 5.  The copies are step 5's: n == 1 gives V[0]; not wrap, i < 0 gives
 *       V[0]; not wrap, i == n-1 gives V[n-1].  (Deviation: Godot evaluates the cubic at c = 0 there,
 *       the same value but for -0 and non-finite bits.)
 *       Keys, not wrap (interior i): a = i, b = i+1, pre = max(i-1, 0), post = min(i+2, n-1);
 *       pre_t = (float)(T[pre] - T[a]), to_t = (float)(T[b] - T[a]), post_t = (float)(T[post] - T[a]).
 *       Keys, wrap: a = i, or n-1 when i < 0; b = (a+1) mod n, pre = (a-1) mod n, post = (a+2) mod n;
 *       pre_t = pre > a ? (float)((-length + T[pre]) - T[a]) : (float)(T[pre] - T[a]);
 *       to_t = b < a ? (float)((length + T[b]) - T[a]) : (float)(T[b] - T[a]);
 *       post_t = (b < a || post <= a) ? (float)((length + T[post]) - T[a]) : (float)(T[post] - T[a]).
 *       (At n == 2 and n == 3 pre and post alias a and b, or wrap onto them.)
 *       c = step 5's weight from / delta with step 5's delta and its three cases (interior,
 *       i == n-1, i < 0) -- Godot computes to_t and delta separately, and so does this.
 *       cubic(from, to, pre, post) (Barry-Goldman):
 *         t  = lerp(0, to_t, c)
 *         a1 = lerp(pre, from, pre_t == 0 ? 0 : (t - pre_t) / -pre_t)
 *         a2 = lerp(from, to, to_t == 0 ? 0.5 : t / to_t)
 *         a3 = lerp(to, post, post_t - to_t == 0 ? 1 : (t - to_t) / (post_t - to_t))
 *         b1 = lerp(a1, a2, to_t - pre_t == 0 ? 0 : (t - pre_t) / (to_t - pre_t))
 *         b2 = lerp(a2, a3, post_t == 0 ? 1 : t / post_t)
 *         result lerp(b1, b2, to_t == 0 ? 0.5 : t / to_t)
 *       Position, scale and shape values: c == 0 (-0 included; a time exactly on key a, or a
 *       delta below CMP_EPSILON) gives V[a]'s bits, copied; otherwise cubic(V[a], V[b], V[pre],
 *       V[post]) per component; step 6.  (Deviation: Godot evaluates the scheme at c == 0 too, whose
 *       result lerp(pre + (from - pre), from, w) is `from` only when from - pre is a float32 and is
 *       within an ulp of max(|from - pre|, |from|) of it otherwise.)  The rotation has no such rule.
 *       Rotation, the key quaternions used as given:
 *         from, pre, to, post = Basis(q).get_rotation_quaternion() of V[a], V[pre], V[b], V[post];
 *         pre = signbit(dot(from, pre)) ? -pre : pre;
 *         flip2 = signbit(dot(from, to)); to = flip2 ? -to : to;
 *         flip3 = flip2 ? dot(to, post) <= 0 : signbit(dot(to, post)); post = flip3 ? -post : post;
 *         log(q) = get_axis(q) * angle(q) as (x, y, z, 0), angle(q) = 2 * (w < -1 ? pi : (w > 1 ? 0 :
 *         acosf(w))) (Math::acos clamps);
 *         exp(v): theta = length(v), u = normalized(v); identity when theta < CMP_EPSILON or u is not
 *         normalized (length_squared(u) != 1 and not |length_squared(u) - 1| < 0.001, UNIT_EPSILON);
 *         otherwise Quaternion(u, theta);
 *         q1 = from * exp(L1), L1.xyz = cubic(0, log(from^-1 * to), log(from^-1 * pre), log(from^-1 *
 *         post)) per component; q2 = to * exp(L2), L2.xyz = cubic(log(to^-1 * from), 0, log(to^-1 *
 *         pre), log(to^-1 * post)); ^-1 is the conjugate;
 *         result Quaternion::slerp(q1, q2, c) as in mbik_pose_blend, not renormalised; step 6.
 * Everything else applies to a cubic channel as to a linear one: steps 1 to 4 and 6, the layer rules
 * of mbik_clip_sample_layers, the seam split of mbik_clip_root_motion (at c == 0 the position, scale
 * and shape value is V[a] exactly), the shapes' init.  The device gives mbik_clip_call_cpu's
 * bits.  Not covered: INTERPOLATION_LINEAR_ANGLE / CUBIC_ANGLE, ping-pong, key transitions. */
typedef struct mbik_clipset_desc {
	int32_t struct_size;               /* sizeof(mbik_clipset_desc) */
	int32_t bone_count;
	const float *rest_pose;            /* [bones][10] */
	int32_t clip_count;
	const mbik_clip_desc *clips;       /* a track's interpolation may be 2 */
	const mbik_clipset_shapes *shapes; /* or NULL: a set without shapes */
	int32_t libm_variant;
	uint32_t flags;                    /* 0 */
} mbik_clipset_desc;
int32_t mbik_clipset_create_desc(const mbik_clipset_desc *desc, int32_t device, mbik_clipset **out);

#define MBIK_CLIP_CALL_SAMPLE 0              /* mbik_clip_sample_cpu: count, time, clip_index, clip, out (poses) */
#define MBIK_CLIP_CALL_SAMPLE_LAYERS 1       /* mbik_clip_sample_layers_cpu: count, layer_count, layers, flags, out (poses) */
#define MBIK_CLIP_CALL_SHAPES 2              /* mbik_clip_sample_shapes_cpu: as SAMPLE, out (weights) */
#define MBIK_CLIP_CALL_SHAPES_LAYERS 3       /* mbik_clip_sample_shapes_layers_cpu: as SAMPLE_LAYERS, out (weights) */
#define MBIK_CLIP_CALL_ROOT_MOTION 4         /* mbik_clip_root_motion_cpu: count, root_bone, time_prev, time, clip_index, clip, out (motion), pose */
#define MBIK_CLIP_CALL_ROOT_MOTION_LAYERS 5  /* mbik_clip_root_motion_layers_cpu: count, layer_count, root_bone, layers, time_prev, flags, out, pose */
typedef struct mbik_clip_call {
	int32_t struct_size;           /* sizeof(mbik_clip_call) */
	int32_t kind;                  /* MBIK_CLIP_CALL_* */
	int32_t count;
	int32_t layer_count;
	int32_t root_bone;
	int32_t clip;                  /* used when clip_index is NULL */
	uint32_t flags;
	const double *time;
	const double *time_prev;
	const int32_t *clip_index;
	const mbik_clip_layer *layers;
	float *out;                    /* pose_out, weights_out or motion_out */
	float *pose;                   /* the root-motion kinds: may be NULL */
} mbik_clip_call;
int32_t mbik_clip_call_cpu(const mbik_clipset_desc *set, const mbik_clip_call *call);

/* Linear blend skinning of a mesh from skin transforms (ABI 10): what mbik_pose_globals' skinned
 * output exists for, on the device and on the stream of the solve.  The semantics are those of
 * Godot's skeleton compute shader -- blend the bone matrices, then transform -- on the ArrayMesh
 * surface arrays ARRAY_VERTEX, ARRAY_NORMAL, ARRAY_BONES and ARRAY_WEIGHTS with 4 or 8 influences
 * a vertex.  For vertex v of skeleton s, X_k = skin[s][bone_indices[v][k]], w_k = weights[v][k]:
 *   M = X_0 * w_0, then M = M + X_k * w_k for k = 1 .. K-1 in influence order, every element of the
 *   12 floats and every influence, weight 0 included;
 *   out_positions[s][v] = M * positions[v]  (per row ((r.x*v.x + r.y*v.y) + r.z*v.z) + origin);
 *   out_normals[s][v]   = M.basis * normals[v], the same matrix without the origin, not renormalised.
 * float32, unfused, in that order; mbik_skin_vertices_cpu is the specification (a renderer fixes no
 * float order) and the device gives the same bits.  Weights are used as given: not normalised, not
 * sorted, negative ones and sums other than 1 allowed.  Non-finite values propagate: a NaN in one
 * bone's matrix reaches exactly the vertices that list that bone, also with weight 0.
 *
 * A mesh is its own handle, bound to a bone count and a device, not to a plan: one rig can carry
 * several meshes and one mesh can serve several plans.  mbik_mesh_create reads host arrays --
 *   positions    [vertex_count][3]
 *   normals      [vertex_count][3], or NULL for a mesh without normals
 *   bone_indices [vertex_count][influences]
 *   weights      [vertex_count][influences]
 * -- checks them on the host and copies them, repacked for the kernel, to `device`
 * (synchronously).  MBIK_EINVAL: influences other than 4 or 8, a negative count, a null array of a
 * mesh with vertices, any bone index outside [0, bone_count), a null out_mesh.
 * MBIK_EUNSUPPORTED: bone_count above MBIK_SKIN_MAX_BONES (one skeleton's matrices, 48 bytes a
 * bone, must fit MBIK_MAX_LDS_BYTES).  A mesh is immutable afterwards; the kernel relies on the
 * index check made here and tests no index itself. */
typedef struct mbik_mesh mbik_mesh;
int32_t mbik_mesh_create(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, int32_t device, mbik_mesh **out_mesh);
void mbik_mesh_destroy(mbik_mesh *mesh);
/* Skins the mesh for `count` skeletons.  Device buffers on the mesh's device, asynchronous on
 * hip_stream (NULL = default stream):
 *   skin          [count][bones][12] basis rows, then origin, e.g. mbik_pose_globals' output with
 *                 inv_bind on the same stream
 *   out_positions [count][vertices][3]
 *   out_normals   [count][vertices][3], or NULL
 * MBIK_EINVAL: count < 0, a null skin or out_positions, out_normals for a mesh without normals, an
 * output that overlaps skin or the other output.  count == 0 or a mesh without vertices returns
 * MBIK_OK without a launch.  Buffers need float alignment only (a 16-byte aligned skin is staged
 * 16 bytes a lane).  Element offsets are 64-bit: count x vertices x 3 may exceed 2^31. */
int32_t mbik_skin_vertices(mbik_mesh *mesh, int32_t count, const float *skin, float *out_positions, float *out_normals,
		void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with
 * mbik_mesh_create's and mbik_skin_vertices' checks (any bone count). */
int32_t mbik_skin_vertices_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, int32_t count, const float *skin,
		float *out_positions, float *out_normals);
/* The launch shape mbik_skin_vertices would use for `count` skeletons: a block owns
 * skeletons_per_block consecutive skeletons (their matrices in LDS) and one of vertex_chunks
 * pieces of the vertex range; the grid is skeleton tiles x vertex chunks, so that a small count
 * with a large mesh still fills the device.  Either output may be NULL. */
int32_t mbik_mesh_launch_shape(const mbik_mesh *mesh, int32_t count, int32_t *skeletons_per_block, int32_t *vertex_chunks);

/* Blend shapes (morph targets) in front of the skinning (ABI 13): the first half of Godot 4.3's
 * skeleton compute shader, BLEND_SHAPE_MODE_RELATIVE and BLEND_SHAPE_MODE_NORMALIZED, so that the
 * skeletons of one batch need not be the same body.  A shaped mesh carries P >= 1 shapes --
 *   shapes.positions [shape_count][vertex_count][3]
 *   shapes.normals   [shape_count][vertex_count][3], given exactly when the mesh has normals
 * -- shared by every skeleton, and each skeleton brings P weights.  For vertex v of skeleton s with
 * c_j = shape_weights[s][j], float32, unfused, in this order:
 *   bp = (0,0,0); bn = (0,0,0); total = 0.0f
 *   for j = 0 .. P-1 ascending, if fabsf(c_j) > 0.0001f (the shader's test; false for NaN, so a
 *   NaN weight is skipped):
 *       bp = bp + shapes.positions[j][v] * c_j       (V3 * float, then V3 + V3)
 *       bn = bn + shapes.normals[j][v] * c_j         (meshes with normals only)
 *       total = total + c_j
 *   pos = positions[v]; nrm = normals[v]
 *   mode normalized: base_w = 1.0f - total; pos = pos * base_w; nrm = nrm * base_w
 *   pos = pos + bp
 *   nrm = normalized(nrm + bn)   x / sqrt((x*x + y*y) + z*z) per component with IEEE sqrt and
 *                                division; the zero vector stays zero
 * and mbik_skin_vertices' blend and transform then run on pos and nrm, unchanged.  It follows that
 * with every weight skipped a relative-mode position is positions[v] + (+0,+0,+0) (the base's bits,
 * except that -0 becomes +0), that the normal of a shaped call is always renormalised before the
 * bone transform (the shader's behaviour; mbik_skin_vertices never renormalises), and that
 * infinite weights and non-finite shape data propagate.  mbik_skin_vertices_shaped_cpu is the
 * specification and the device gives the same bits.  Deviations from Godot: the shader reads
 * octahedral-packed normals and compressed vertex formats, here every array is float32; tangents
 * are not covered by this call: mbik_skin_vertices_call below carries them.
 *
 * mbik_mesh_create_shaped is mbik_mesh_create with shapes: the same arguments and checks, plus
 * MBIK_EINVAL for a null `shapes`, a struct_size below sizeof(mbik_mesh_shapes), shape_count < 1,
 * an unknown mode, null shapes.positions on a mesh with vertices, and normals on exactly one of
 * the mesh and the shapes; MBIK_EUNSUPPORTED when bone_count * 48 + shape_count * 4 exceeds
 * MBIK_MAX_LDS_BYTES (one skeleton's matrices and shape weights are staged together).  The shape
 * arrays are copied like the mesh's.  mbik_skin_vertices on a shaped mesh skins the base arrays
 * with that call's semantics and bits, without shapes and without renormalisation;
 * mbik_mesh_launch_shape on a shaped mesh reports what mbik_skin_vertices_shaped would use (the
 * LDS of one skeleton is bone_count * 48 + shape_count * 4 bytes there). */
#define MBIK_SHAPE_MODE_RELATIVE 0
#define MBIK_SHAPE_MODE_NORMALIZED 1
typedef struct mbik_mesh_shapes {
	int32_t struct_size;       /* sizeof(mbik_mesh_shapes) */
	int32_t shape_count;       /* P >= 1 */
	int32_t mode;              /* MBIK_SHAPE_MODE_* */
	const float *positions;    /* [shape_count][vertex_count][3] */
	const float *normals;      /* [shape_count][vertex_count][3], or NULL for a mesh without normals */
} mbik_mesh_shapes;
int32_t mbik_mesh_create_shaped(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes,
		int32_t device, mbik_mesh **out_mesh);
/* mbik_skin_vertices with blend shapes: shape_weights is [count][shape_count] in device memory, read
 * by the kernel, never by the host; the other arguments as for mbik_skin_vertices.  MBIK_EINVAL:
 * a mesh without shapes, null shape_weights with count > 0 and vertices, shape_weights overlapping
 * an output, and everything mbik_skin_vertices refuses.  count == 0 or a mesh without vertices
 * returns MBIK_OK without a launch.  Buffers need float alignment only. */
int32_t mbik_skin_vertices_shaped(mbik_mesh *mesh, int32_t count, const float *skin, const float *shape_weights,
		float *out_positions, float *out_normals, void *hip_stream);
/* Host-only (no device needed): the same arithmetic from the same code on host buffers, with
 * mbik_mesh_create_shaped's and mbik_skin_vertices_shaped's checks except the LDS limit (any bone
 * and shape count). */
int32_t mbik_skin_vertices_shaped_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t count,
		const float *skin, const float *shape_weights, float *out_positions, float *out_normals);

/* Skeleton bounds and frustum culling (ABI 14): which skeletons of a batch can be seen, decided on
 * the device from the skin transforms mbik_pose_globals wrote, without reading them or the skinned
 * vertices back.  The semantics are Godot 4.3's MeshStorage::mesh_get_aabb(mesh, skeleton) -- one box
 * per bone, built when the surface is created (RenderingServer::_surface_set_data), moved by the
 * skeleton's skin transforms and merged -- and the plane half of AABB::intersects_convex_shape,
 * restated here; the _cpu entries are the specification and the device gives the same bits.  All
 * arithmetic is float32, unfused, in the order written.  A box is 6 floats: position x, y, z, then
 * size x, y, z (Godot's AABB).
 *
 * 1. Bone boxes, computed by mbik_mesh_create and mbik_mesh_create_shaped from the arrays they
 * validate (no further failure case: a call that succeeded before ABI 14 still does):
 *   for v ascending, for k = 0 .. influences-1:
 *     w = weights[v][k]; b = bone_indices[v][k]; p = positions[v]
 *     if (w == 0) continue                          +0 and -0 are skipped; NaN and negative weights count
 *     if bone b is not yet used: box[b] = { p, (1e-5f, 1e-5f, 1e-5f) }; used[b] = 1
 *     else (AABB::expand_to): begin = box[b].position; end = box[b].position + box[b].size
 *                             per axis: if (p < begin) begin = p; if (p > end) end = p
 *                             box[b] = { begin, end - begin }
 * A NaN coordinate fails both compares, so it changes nothing after the first hit; as a first hit
 * it is stored as given.  An unused bone has used = 0 and a box of six zeros (Godot marks it with
 * size (-1,-1,-1); the flag is the same information without a magic value).  Blend shapes do not
 * enter the boxes -- Godot's behaviour, and the reason it has extra_cull_margin; `margin` of
 * mbik_cull_boxes is the remedy.  The mesh keeps the used bones' boxes on its device in a table of
 * its own.  mbik_mesh_bone_boxes copies the boxes out: boxes [bone_count][6], used [bone_count],
 * host memory.  mbik_bone_boxes_cpu is the host-only form with mbik_mesh_create's checks (any bone
 * count); MBIK_EINVAL also for a null boxes or used with bone_count > 0. */
int32_t mbik_mesh_bone_boxes(const mbik_mesh *mesh, float *boxes, uint8_t *used);
int32_t mbik_bone_boxes_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const int32_t *bone_indices, const float *weights, float *boxes, uint8_t *used);
/* 2. One box per skeleton.  For skeleton s, over the used bones j in ascending order:
 *   t = xform_aabb(skin[s][j], box[j])              Transform3D::xform(AABB):
 *         mn = box.position; mx = box.position + box.size
 *         for row i: lo = hi = origin[i]
 *           for column c = 0..2: e = basis[i][c] * mn[c]; f = basis[i][c] * mx[c]
 *                                if (e < f) { lo += e; hi += f } else { lo += f; hi += e }
 *         t = { lo, hi - lo }
 *   first used bone: acc = t
 *   otherwise (AABB::merge_with): e1 = acc.size + acc.position; e2 = t.size + t.position
 *         per axis: mn = acc.position < t.position ? acc.position : t.position
 *                   mx = e1 > e2 ? e1 : e2
 *         acc = { mn, mx - mn }
 * and boxes[s] = acc.  A mesh without a used bone (or without vertices) writes six zeros; Godot
 * falls back to the surface's static box there (a stated deviation).  Non-finite values go where
 * those compares send them (no fminf / fmaxf).  The merge is a chain, not a reduction: every step
 * re-derives the end from the rounded size, so the bits are those of the ascending order and of no
 * other.  Device buffers on the mesh's device, asynchronous on hip_stream (NULL = default stream):
 *   skin   [count][bones][12], e.g. mbik_pose_globals' output with inv_bind on the same stream
 *   boxes  [count][6]
 * MBIK_EINVAL: a null mesh, count < 0, a null skin or boxes, boxes overlapping skin.  count == 0
 * returns MBIK_OK without a launch.  Buffers need float alignment only; element offsets are 64-bit.
 * mbik_skin_bounds_cpu is the host-only form: bone_boxes [bone_count][6] and used [bone_count] as
 * mbik_mesh_bone_boxes gives them, any bone count. */
int32_t mbik_skin_bounds(mbik_mesh *mesh, int32_t count, const float *skin, float *boxes, void *hip_stream);
int32_t mbik_skin_bounds_cpu(int32_t bone_count, const float *bone_boxes, const uint8_t *used, int32_t count, const float *skin,
		float *boxes);
/* 3. The plane test and the ordered visible list.  For skeleton s, in this order:
 *   (p, z) = boxes[s]
 *   if skeleton_global: (p, z) = xform_aabb(skeleton_global[s], p, z)     to world space, as in 2.
 *   if (margin != 0): p = p - margin; z = z + margin * 2.0f               Godot's extra_cull_margin
 *   e = p + z
 *   for each plane i ascending (normal n, distance d; the normal points out of the frustum):
 *     c = (n.x > 0 ? p.x : e.x, n.y > 0 ? p.y : e.y, n.z > 0 ? p.z : e.z)   the corner with the least n.x
 *     if (((n.x*c.x + n.y*c.y) + n.z*c.z) > d): culled, stop                Plane::is_point_over
 *   otherwise visible
 * A box that touches a plane (the dot product equals d) is visible.  A NaN anywhere fails the
 * compare, so such a skeleton stays visible: the conservative side.  plane_count == 0 makes every
 * skeleton visible.  Device buffers on the mesh's device except `planes`:
 *   boxes           [count][6], e.g. mbik_skin_bounds' output on the same stream
 *   skeleton_global [count][12] basis rows, then origin, as in mbik_capture_targets, or NULL
 *   planes          HOST [plane_count][4]: normal x, y, z, then d; copied at the call into the
 *                   kernels' arguments, so the call stays asynchronous and the array may be reused at once
 *   visible         [count] bytes, 0 or 1, or NULL
 *   indices         [count], or NULL: indices[0 .. n) are the visible s in ascending order (the same
 *                   list on every run); indices[n ..] is not touched
 *   visible_count   [1]: n, written by every call (the caller does not clear it); required with
 *                   indices, optional without
 * Asynchronous on hip_stream.  The mesh gives the device and owns the scratch for the per-block
 * counts behind the list, so calls on one mesh are stream-ordered (use one stream per mesh, or order
 * the streams); the scratch grows with the largest count seen, and growing it waits for the device.
 * MBIK_EINVAL: a null mesh, null boxes with count > 0, count < 0, plane_count outside
 * [0, MBIK_CULL_MAX_PLANES], null planes with plane_count > 0, visible and indices both NULL, indices
 * without visible_count, an output overlapping an input or another output.  count == 0 writes
 * visible_count[0] = 0 when given and launches nothing else.  mbik_cull_boxes_cpu is the same on
 * host buffers, without a mesh. */
#define MBIK_CULL_MAX_PLANES 16
int32_t mbik_cull_boxes(mbik_mesh *mesh, int32_t count, const float *boxes, const float *skeleton_global, float margin,
		int32_t plane_count, const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count, void *hip_stream);
int32_t mbik_cull_boxes_cpu(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count);
/* 4. Distance LOD lists: one ordered list per visibility range, so that each level of detail of a
 * character -- a mesh of its own -- skins the skeletons in its distance band and no others
 * (mbik_skin_vertices_listed takes each list as it is).  Additive: nothing that existed changed,
 * MBIK_ABI_VERSION stays 15, and a caller detects the feature by the presence of the symbol
 * mbik_cull_lod (dlsym, or MBIK_LOD_MAX_RANGES at compile time).
 *
 * Semantics -- Godot's core is not part of the reference tree, so mbik_cull_lod_cpu is the
 * specification and the device gives the same bits.  It is modelled on Godot 4.3's
 * RendererSceneCull::_visibility_range_check with VISIBILITY_RANGE_FADE_DISABLED
 * (GeometryInstance3D.visibility_range_begin / _end and their margins), placed in front of step 3's
 * plane test.  A range is mbik_lod_range; a 0 in begin or end means no limit on that side.  For
 * skeleton s, in this order:
 *   (p, z) = boxes[s], then skeleton_global and margin, exactly as in 3.; vis = 3.'s verdict for it
 *   c = p + z * 0.5f                                                         AABB::get_center
 *   v = c - camera; dist = sqrt((v.x*v.x + v.y*v.y) + v.z*v.z)              Vector3::distance_to
 *   for each range r ascending: prev = (state[s] >> r) & 1                   in range r last time?
 *     bo = -begin_margin; eo = end_margin; if (!prev) { bo = -bo; eo = -eo }
 *     in_r = !(end > 0 && dist > end + eo) && !(begin > 0 && dist < begin + bo)
 *   state[s] = bit r is in_r for r < range_count, 0 above
 *   level[s] = the least r with vis && in_r, or MBIK_LOD_NONE
 * Each sum is one float32 addition.  The margins are the hysteresis: a skeleton that was inside a
 * range stays until it is a margin past the edge, one that was outside enters only a margin inside
 * it.  A NaN dist fails both compares, so such a skeleton is in every range: the conservative side,
 * as in the plane test.  state is written for every skeleton, whatever vis is: the engine runs its
 * visibility-range pass over all range-carrying instances before the frustum test, and so a skeleton
 * that comes back into view has the state of where it is, not of where it left.  A caller starts
 * with zeros for strict entry (a skeleton inside a margin may be in no range for that frame) or with
 * 0xFF for lenient entry, and keeps the buffer from frame to frame.
 * List r is indices[r * count + 0 .. n_r), n_r = list_counts[r]:
 *   without MBIK_LOD_EXCLUSIVE  the s with vis && in_r; ranges may overlap, so a skeleton may be in
 *                               several lists
 *   with MBIK_LOD_EXCLUSIVE     the s with level[s] == r: the lists are disjoint
 * in ascending order, the same list on every run.  list_counts[r] is written by every call (the
 * caller does not clear it); entries at and past n_r are not touched; the row stride is count and
 * offsets are 64-bit.  With range_count == 1, ranges[0] all zero and any state, list 0 and its count
 * are mbik_cull_boxes' indices and visible_count bit for bit.
 * Deviations from the engine, stated: no fade modes (Godot turns the margins into alpha there), no
 * visibility_parent dependencies, no per-viewport state, state advances for frustum-culled skeletons
 * too, and the centre is that of the margin-grown box.
 * Device buffers on the mesh's device except planes, camera and ranges:
 *   boxes, skeleton_global, margin, plane_count, planes    as for mbik_cull_boxes
 *   camera       HOST [3]: the camera's world position
 *   ranges       HOST [range_count]; planes, camera and ranges are copied at the call into the
 *                kernels' arguments, so the call stays asynchronous and they may be reused at once
 *   state        [count] bytes, read and written
 *   level        [count] bytes, or NULL
 *   indices      [range_count][count]
 *   list_counts  [range_count]
 * Asynchronous on hip_stream.  The mesh gives the device and owns the scratch only (the per-block
 * counts, shared with mbik_cull_boxes, and one byte a skeleton), so a LOD set passes its first
 * mesh, and calls on one mesh are stream-ordered; growing the scratch waits for the device.
 * MBIK_EINVAL: everything mbik_cull_boxes refuses for the arguments the two share (a null mesh,
 * count < 0, plane_count outside [0, MBIK_CULL_MAX_PLANES], null planes with plane_count > 0, null
 * boxes with count > 0), range_count outside [1, MBIK_LOD_MAX_RANGES], a null ranges or camera, a
 * non-finite camera, a range with a non-finite or negative field or with end > 0 && begin > end,
 * unknown flag bits, with count > 0 a null state, indices or list_counts, any output overlapping an
 * input or another output (state is both, and may overlap nothing else).  count == 0 writes
 * range_count zeros to list_counts when given and launches nothing else.  mbik_cull_lod_cpu is the
 * same on host buffers, without a mesh. */
typedef struct mbik_lod_range {
	float begin, end;               /* visibility_range_begin / _end; 0 = no limit on that side */
	float begin_margin, end_margin; /* visibility_range_begin_margin / _end_margin */
} mbik_lod_range;                   /* 16 bytes */
#define MBIK_LOD_MAX_RANGES 8
#define MBIK_LOD_EXCLUSIVE 1u
#define MBIK_LOD_NONE 255
int32_t mbik_cull_lod(mbik_mesh *mesh, int32_t count, const float *boxes, const float *skeleton_global, float margin,
		int32_t plane_count, const float *planes, const float *camera, int32_t range_count, const mbik_lod_range *ranges,
		uint32_t flags, uint8_t *state, uint8_t *level, int32_t *indices, int32_t *list_counts, void *hip_stream);
int32_t mbik_cull_lod_cpu(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, const float *camera, int32_t range_count, const mbik_lod_range *ranges, uint32_t flags, uint8_t *state,
		uint8_t *level, int32_t *indices, int32_t *list_counts);

/* List-driven skinning (ABI 15): the skeletons a device-resident list names -- mbik_cull_boxes'
 * indices and visible_count on the same stream are such a list -- skinned without a host read-back
 * of the list or its length.  mbik_skin_vertices_listed_cpu is the specification and the device gives
 * the same bits:
 *   n = min(max(list_count[0], 0), max_list)       list_count is read on the device, never by the host
 *   for r = 0 .. n-1:  s = indices[r]
 *     if (s < 0 || s >= count) continue             the entry is skipped: nothing is read or written for it
 *     row = (flags & MBIK_SKIN_LIST_COMPACT) ? r : s
 *     out_positions[row][v], out_normals[row][v], all v  =  what mbik_skin_vertices (shape_weights NULL) or
 *         mbik_skin_vertices_shaped (shape_weights given) writes to row s for skin[s] (and shape_weights[s]),
 *         bit for bit
 *   every other row of the outputs is not touched
 * Device buffers on the mesh's device, asynchronous on hip_stream (NULL = default stream):
 *   indices       [max_list]; need not be ascending or unique.  A duplicate writes the same bits twice
 *                 in place and one row each when compact; entries at and past n are not read
 *   list_count    [1]: the list's length
 *   max_list      HOST: an upper bound on the length, which sizes the launch; it may exceed count
 *   skin          [count][bones][12], as for mbik_skin_vertices
 *   shape_weights [count][shape_count], or NULL: a NULL on a shaped mesh skins the base arrays, as
 *                 mbik_skin_vertices does
 *   out_positions, out_normals (or NULL)
 *                 in place [count][vertices][3]; compact [max_list][vertices][3], row r belonging to
 *                 skeleton indices[r], so the caller's instance map is the list itself
 * The mesh's own bone indices are checked once by the host when the mesh is created; this list is
 * device data the host never sees, so here the kernel tests every entry against [0, count) itself.
 * MBIK_EINVAL: everything mbik_skin_vertices or mbik_skin_vertices_shaped refuses (a null mesh,
 * count < 0, a null skin or out_positions, out_normals for a mesh without normals, an output that
 * overlaps skin, shape_weights or the other output), a negative max_list, unknown flag bits, a
 * non-null shape_weights on a mesh without shapes, null indices or list_count with work to do, an
 * output overlapping indices or list_count; output sizes follow the flag.  count == 0, max_list == 0
 * or a mesh without vertices returns MBIK_OK without a launch.  Buffers need float alignment only;
 * element offsets are 64-bit.  The launch shape is mbik_mesh_launch_shape's for max_list skeletons
 * (of the plain call when shape_weights is NULL): a block owns that many consecutive list entries.
 * The _cpu form takes mbik_skin_vertices_shaped_cpu's mesh arguments (any bone and shape count);
 * `shapes` may be NULL for a mesh without shapes, and every buffer is host memory. */
#define MBIK_SKIN_LIST_COMPACT 1u
int32_t mbik_skin_vertices_listed(mbik_mesh *mesh, int32_t count, const int32_t *indices, const int32_t *list_count,
		int32_t max_list, const float *skin, const float *shape_weights, uint32_t flags, float *out_positions,
		float *out_normals, void *hip_stream);
int32_t mbik_skin_vertices_listed_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t count,
		const int32_t *indices, const int32_t *list_count, int32_t max_list, const float *skin, const float *shape_weights,
		uint32_t flags, float *out_positions, float *out_normals);

/* The tangent stream, and one struct-based call over the plain, the shaped and the listed form
 * (additive to ABI 15: MBIK_ABI_VERSION stays 15, look the symbols up by name; every entry point above
 * keeps its signature, checks, texts and bits).  Godot 4.3's skeleton compute shader carries
 * ARRAY_TANGENT through the same two steps as the normal, the blend-shape pass and the bone
 * transform; so does this call.  A mesh described by mbik_mesh_desc may have tangents [V][4]: xyz and
 * the binormal sign w.  mbik_skin_vertices_call_cpu is the specification and the device gives the same
 * bits.
 *
 * With out_tangents == NULL the call IS the existing entry of the same form -- mbik_skin_vertices when
 * indices, list_count and shape_weights are NULL, mbik_skin_vertices_shaped when only shape_weights is
 * given, mbik_skin_vertices_listed when the list is given: the same bits, the same refusals with the
 * same texts, the same kernels.  With out_tangents, for vertex v of the skeleton written to row `row`,
 * m the blended matrix the position and the normal use, t = tangents[v], float32, unfused, in this
 * order:
 *   shaped call only (shape_weights given):
 *     bt = (0,0,0); inside the ascending loop over the active shapes  bt = bt + shape_tangents[j][v] * c_j
 *     mode normalized: t.xyz = t.xyz * base_w
 *     t.xyz = normalized(t.xyz + bt)                 as the normal's: the zero vector stays zero
 *   every form:
 *     out_tangents[row][v].xyz = m.basis * t.xyz     the normal's transform, not renormalised
 *     out_tangents[row][v].w   = the bits of tangents[v][3], copied and never computed with
 * A plain or listed call without shape_weights on a shaped mesh uses the base tangents without
 * renormalisation, as the normals.  Deviations from Godot, as before: no octahedral packing, float32
 * arrays, and the tangent is not re-orthogonalised against the skinned normal.
 *
 * mbik_mesh_create_desc is mbik_mesh_create (shapes NULL) or mbik_mesh_create_shaped with the same
 * checks, and MBIK_EINVAL for a null desc, a struct_size below sizeof(mbik_mesh_desc), tangents
 * without normals, and shape_tangents on exactly one side of (shapes and tangents both given).  On the
 * device the tangents lie behind every other plane of the mesh: a mesh without them is the image it
 * always was.
 *
 * mbik_skin_vertices_call: device buffers on the mesh's device, asynchronous on hip_stream.
 * MBIK_EINVAL: a null call, a struct_size below sizeof(mbik_skin_call), a null mesh, exactly one of
 * indices and list_count given, out_tangents on a mesh without tangents, out_tangents without
 * out_normals, out_tangents (rows x vertices x 16 bytes) overlapping skin, shape_weights, indices,
 * list_count or another output, and everything the matching existing entry refuses.  rows is count,
 * or max_list for a compact list.  count == 0, max_list == 0 in the listed form or a mesh without
 * vertices returns MBIK_OK without a launch.  Buffers need float alignment only; element offsets
 * are 64-bit ((row * vertices + v) * 4 passes 2^31 sooner than the other outputs' x 3).  The _cpu
 * form takes the mesh as its descriptor (any bone and shape count) with the same checks and texts;
 * every buffer is host memory. */
typedef struct mbik_mesh_desc {
	int32_t struct_size;               /* sizeof(mbik_mesh_desc) */
	int32_t bone_count, vertex_count, influences;
	const float *positions;            /* [V][3] */
	const float *normals;              /* [V][3] or NULL */
	const float *tangents;             /* [V][4] xyz + binormal sign w, or NULL; needs normals */
	const int32_t *bone_indices;       /* [V][K] */
	const float *weights;              /* [V][K] */
	const mbik_mesh_shapes *shapes;    /* or NULL */
	const float *shape_tangents;       /* [P][V][3]; given exactly when shapes and tangents both are */
} mbik_mesh_desc;
int32_t mbik_mesh_create_desc(const mbik_mesh_desc *desc, int32_t device, mbik_mesh **out_mesh);

typedef struct mbik_skin_call {
	int32_t struct_size;               /* sizeof(mbik_skin_call) */
	int32_t count;
	const float *skin;                 /* [count][bones][12] */
	const float *shape_weights;        /* [count][P] or NULL */
	const int32_t *indices;            /* both NULL: the range call over rows 0 .. count-1 */
	const int32_t *list_count;
	int32_t max_list;                  /* as mbik_skin_vertices_listed; ignored for the range call */
	uint32_t flags;
	float *out_positions, *out_normals; /* [rows][V][3] */
	float *out_tangents;               /* [rows][V][4] or NULL; needs out_normals */
} mbik_skin_call;
int32_t mbik_skin_vertices_call(mbik_mesh *mesh, const mbik_skin_call *call, void *hip_stream);
int32_t mbik_skin_vertices_call_cpu(const mbik_mesh_desc *desc, const mbik_skin_call *call);

/* Heterogeneous batches: several plans (distinct rigs, e.g. a crowd of different characters)
 * solved by ONE launch, each plan with its own layout.  The reference runs one
 * ManyBoneIK3D::_process_modification per rig (many_bone_ik_3d.cpp:645-694); a group is
 * that loop over rigs, fused.  Plans stay owned by the caller and must outlive the group;
 * all on one device.  constraint_mode and pinless plans run their own launches in order. */
int32_t mbik_group_create(mbik_plan *const *plans, int32_t n_plans, mbik_group **out_group);
/* One frame of every plan in the group: per plan i, skeletons [first[i], first[i]+count[i])
 * (first NULL = 0, count NULL = the plan's skeleton count), device buffers pose_in[i],
 * targets[i], pose_out[i] as for mbik_solve.  Asynchronous on hip_stream; calls on one group
 * are stream-ordered (use one stream per group). */
int32_t mbik_group_solve(mbik_group *group, const int32_t *first, const int32_t *count, const float *const *pose_in,
		const float *const *targets, float *const *pose_out, void *hip_stream);
void mbik_group_destroy(mbik_group *group);

/* Multi-GPU in one process (ABI 8): one batch of skeletons sharded over several
 * plans, typically one per GPU, for an engine that is a single process (Godot is): contiguous
 * shards in plan order -- plan i owns skeletons [off_i, off_i + N_i) of the batch, off_i the sum
 * of the earlier plans' skeleton counts -- solved concurrently, each on its plan's device, with
 * the poses gathered to the root device by peer copies over xGMI (no collective library: the
 * solve has no exchange step).  The plans must agree on bone and pin counts (any topology,
 * layout or setup data otherwise) and stay owned by the caller; they must outlive the handle and
 * must not be solved elsewhere while a mbik_multi_solve on them is in flight.
 *   flags MBIK_MULTI_STAGE_ALL: stage every shard through the handle's own device buffers, even a
 *   shard whose plan lives on the root device (the copy path a one-GPU machine can test). */
#define MBIK_MULTI_STAGE_ALL 1u
int32_t mbik_multi_create(mbik_plan *const *plans, int32_t n_plans, int32_t root_device, uint32_t flags, mbik_multi **out);
/* One frame of the whole batch.  pose_in / targets / pose_out are device buffers on the root
 * device holding every skeleton ([total][bones][10], [total][pins][12]; pose_out may equal
 * pose_in).  Asynchronous on root_stream (a stream of the root device, NULL = its default
 * stream): each plan's work -- the copy of its shard to its device, its mbik_solve, the copy of
 * its poses back into pose_out -- runs on a stream the handle owns on the plan's device, after
 * everything already queued on root_stream, and root_stream waits for all of them, so work
 * queued after the call sees the gathered poses.  Shards whose plan lives on the root device
 * solve in place in the caller's buffers (unless MBIK_MULTI_STAGE_ALL).  Calls on one handle are
 * ordered by root_stream; use one root stream per handle.  Returns the first error; a helper-wave
 * timeout of any plan is reported as by mbik_solve.  Shards run in plan order and the first
 * failing shard ends the call: pose_out is then defined only for the shards before it, and
 * root_stream still waits for everything the call queued (so the buffers are free to reuse once
 * root_stream reaches that point). */
int32_t mbik_multi_solve(mbik_multi *multi, const float *pose_in, const float *targets, float *pose_out, void *root_stream);
/* The batch size (the plans' skeleton counts summed) and shard offsets (off[n_plans + 1],
 * may be NULL). */
int64_t mbik_multi_skeletons(const mbik_multi *multi, int64_t *off);
void mbik_multi_destroy(mbik_multi *multi);

/* Runs IKBoneSegment3D::segment_solver() once on `segment` (index in post-order segment
 * numbering of mbik_plan_segment_table) for every skeleton in [first, first+count), updating
 * pose_inout in place (device pointers).  No pose write-back conversion is skipped: the
 * output is the Skeleton3D pose of every IK bone after that call.
 * segment_solver's other arguments are not parameters here:
 *   p_damp / p_default_damp / p_constraint_mode  come from the plan (mbik_config's bone_damp,
 *                         default_damp, constraint_mode), as the reference passes its own
 *                         members (many_bone_ik_3d.cpp:685-693);
 *   p_current_iteration / p_total_iteration  are accepted by segment_solver but never reach
 *                         _set_optimal_rotation (ik_bone_segment_3d.cpp:94 calls it without them,
 *                         so its slerp weight is always 0 and every iteration is alike); the
 *                         solve has no use for them, and a caller that tracks them loses nothing. */
int32_t mbik_segment_solve(mbik_plan *plan, int32_t segment, int32_t first, int32_t count, float *pose_inout,
		const float *targets, void *hip_stream);
/* Segment table: for each segment, its root bone, tip bone and parent segment (-1). */
int32_t mbik_plan_segment_table(const mbik_plan *plan, int32_t *root_bone, int32_t *tip_bone, int32_t *parent_segment,
		int32_t capacity);
/* Row-uniform bone-step classes of the plan's current schedule (diagnostics and tests): row_steps
 * receives each schedule row's bone-step count (row_capacity entries), classes the class id of
 * every (row, step) in row order (class_capacity entries): 0 where the row's roles take the
 * general bone-step, else the specialised shape every one of them has there.  Derived from the
 * schedule, never stored in a plan file.  Returns the row count.  mbik_describe_step_classes is
 * the host-only form (no device needed) for `desc` at lanes_per_skeleton lanes (0 = automatic). */
int32_t mbik_plan_step_classes(const mbik_plan *plan, int32_t *row_steps, int32_t row_capacity, int32_t *classes,
		int32_t class_capacity);
int32_t mbik_describe_step_classes(const mbik_skeleton_desc *desc, const mbik_config *config, int32_t lanes_per_skeleton,
		int32_t *row_steps, int32_t row_capacity, int32_t *classes, int32_t class_capacity);

/* Host-only (no device needed): runs the _bone_list_changed segmentation for `desc` and
 * reports the solve order.  bone_list receives ManyBoneIK3D::bone_list (capacity
 * bone_count), segment_* receive the post-order segment table (capacity bone_count), and
 * segment_headings the heading count of each segment.  Returns the segment count. */
int32_t mbik_describe_topology(const mbik_skeleton_desc *desc, const mbik_config *config, int32_t *bone_list,
		int32_t *bone_list_count, int32_t *segment_root, int32_t *segment_tip, int32_t *segment_parent,
		int32_t *segment_headings);

/* Device self-test of the kernel's own float primitives against the compiler's IEEE ones,
 * over every float bit pattern (2^32 inputs, ~1 s): out[0] = inputs where the solve's square
 * root differs from the correctly rounded sqrtf (non-NaN results), out[1] = inputs where
 * exactly one of them is NaN.  Both must be 0 (gd_math.h: gd_sqrt). */
int32_t mbik_selftest_math(int32_t device, uint64_t out[2]);

/* Device known-answer tests (ABI 8): the solve kernel's own device functions on the inputs of
 * the reference's unit tests (tests/test_qcp.h:40-113, tests/test_ik_kusudama_3d.h:38-156,
 * tests/test_ik_node_3d.h:39-106), so the HIP code itself -- not only the CPU oracle -- is
 * checked against their expectations.
 * mbik_selftest_qcp: QCP::weighted_superpose + get_translation (qcp.cpp:220-248, 135-137) of n
 *   pairs (moved, target: [n][3]; weights [n]), with eigenvector precision `precision` (the solve
 *   uses 1e-6, ik_bone_segment_3d.h:85), through the primitives of the solve's one-lane heading
 *   branch: out[0..3] the rotation (x, y, z, w), out[4..6] the translation; out[7..13] the same
 *   from the select-form normalizations of the one-wave builds.
 * mbik_selftest_point_in_limits: IKKusudama3D::get_local_point_in_limits (ik_kusudama_3d.cpp:
 *   273-332) through the solve's own local_point_in_limits on the plan's setup tables (constraint
 *   slot `slot`, i.e. the slot-th constraint on a bone of the IK bone list, of skeleton
 *   `skeleton`): out[0..2] / in_bounds[0] the plain form, out[3..5] / in_bounds[1] the select form.
 * mbik_selftest_xform: Transform3D as the IKNode3D tree uses it (ik_node_3d.cpp:56-113), 12 floats
 *   (basis rows, origin): op 0 out = a * b, op 1 out = a.affine_inverse() (b unused). */
int32_t mbik_selftest_qcp(int32_t n, const float *moved, const float *target, const double *weights, int32_t translate,
		double precision, int32_t device, float out[14]);
int32_t mbik_selftest_point_in_limits(const mbik_plan *plan, int32_t slot, int32_t skeleton, const float point[3], float out[6],
		double in_bounds[2]);
int32_t mbik_selftest_xform(int32_t op, const float a[12], const float b[12], int32_t device, float out[12]);

/* Device self-test of the kernel's float quotients (gd_math.h: an fp64 reciprocal with a
 * residual correction, or one rounding for power-of-two numerators) against IEEE division:
 * out[c] = mismatching results of class c below (two NaNs compare equal), out[8 + 2c] and
 * out[9 + 2c] the operand bit patterns of one mismatch.  All counts must be 0.
 *   SPECIALS          every pair of 24 special values (zeros, infinities, NaNs, denormals, extremes)
 *   ALL_DIVIDENDS     all 2^32 dividends for 12 divisors
 *   RANDOM            random_iterations x 2^21 random pairs (free and close exponents)
 *   MIDPOINTS         random_iterations x 2^21 constructed denormal midpoint quotients
 *   POW2_NUMERATOR    0.5 / b, 1 / b, 2 / b for all 2^32 divisors
 *   NORMALIZE         a / sqrtf(l) (normalized()) and the root itself for all 2^32 l, 8 values of a */
#define MBIK_DIV_SPECIALS 0
#define MBIK_DIV_ALL_DIVIDENDS 1
#define MBIK_DIV_RANDOM 2
#define MBIK_DIV_MIDPOINTS 3
#define MBIK_DIV_POW2_NUMERATOR 4
#define MBIK_DIV_NORMALIZE 5
int32_t mbik_selftest_div(int32_t device, uint64_t random_iterations, uint64_t out[20]);

/* Device self-test of the solve's transcendental call sites against values the caller
 * computed with the host's libm (the reference's: Godot's Math::sin/cos/acos call ::sinf,
 * ::cosf, ::acosf and ::sin/::cos; glibc on Linux x86-64).  For fn = SINF, COSF, ACOSF,
 * SLERP_SCALE0 and COS_F64_OF_F32 the inputs are the float bit patterns first ..
 * first+count-1 (first + count <= 2^32); for COS_F64 they are `inputs` (device, count
 * doubles).  expected (device): count floats (SINF..SLERP_SCALE0) or doubles (the two COS
 * variants).  out[0] = results whose bits differ (two NaNs compare equal), out[1] = the
 * lowest differing index (~0 when none).  Synchronizes hip_stream.
 *   SINF, COSF, ACOSF    sin_f / cos_f / acos_f of gd_math.h (glibc 2.35 restated)
 *   SLERP_SCALE0         (float)(sin((double)w) / (double)sinf(w)): Quaternion::slerp's
 *                        weight-0 coefficient (ik_bone_segment_3d.cpp:148-151)
 *   COS_F64_OF_F32       cos((double)x): a cone radius cosine (ik_open_cone_3d.h:47-56)
 *   COS_F64              cos(x): tangent-radius cosines (ik_open_cone_3d.cpp:36-120)
 *   SINF_SSE2, COSF_SSE2, SLERP_SCALE0_SSE2   the same for a plan created with
 *                        libm_variant = MBIK_LIBM_VARIANT_SSE2 (compare with a host libm
 *                        whose FMA ifunc is disabled: GLIBC_TUNABLES=glibc.cpu.hwcaps=-FMA,-AVX2_Usable)
 *   ACOSF_UNIT           the slerp's acosf call site: the branch-free form for -0.5 < x < 1,
 *                        acosf elsewhere; compare with the host acosf */
#define MBIK_LIBM_SINF 0
#define MBIK_LIBM_COSF 1
#define MBIK_LIBM_ACOSF 2
#define MBIK_LIBM_SLERP_SCALE0 3
#define MBIK_LIBM_COS_F64_OF_F32 4
#define MBIK_LIBM_COS_F64 5
#define MBIK_LIBM_SINF_SSE2 6
#define MBIK_LIBM_COSF_SSE2 7
#define MBIK_LIBM_SLERP_SCALE0_SSE2 8
#define MBIK_LIBM_ACOSF_UNIT 9
int32_t mbik_selftest_libm(int32_t fn, uint64_t first, uint64_t count, const double *inputs, const void *expected,
		uint64_t out[3], void *hip_stream);

const char *mbik_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MBIK_H */
