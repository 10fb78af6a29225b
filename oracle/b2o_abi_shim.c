/* b2o_abi_shim.c - TEST INFRASTRUCTURE. Exposes the CPU oracle (b2o_*) under the product's C-ABI
 * symbol names (include/b2hip.h) so that the SAME drop-in Box2D host layer and the SAME scene
 * harness (in box2d-mt_amd/harness) can be linked against the oracle instead of libb2hip.so:
 *   oracle/libb2oracle_harness.so = harness.cpp + box2d-mt_amd/host/src/ (all .cpp) + this shim + b2o_*.c
 * Nothing in the product links this file. */
#include "b2o.h"
#include "../include/b2hip.h"

#include <stdlib.h>
#include <string.h>

struct b2hip_world
{
	b2o_world* o;
	int fixtures;
	int sub_stepping;
	b2hip_should_collide_batch_fn filterBatch; /* asked pair by pair (the oracle decides inline): batches of one */
	void* filterBatchUser;
};

const char* b2hip_last_error(void) { return "cpu oracle shim"; }
const char* b2hip_version(void) { return "b2o oracle shim"; }

int b2hip_world_create(const b2hip_world_def* def, b2hip_world** out)
{
	b2hip_world* w = (b2hip_world*)calloc(1, sizeof(b2hip_world));
	w->o = b2o_world_create(def->gravity_x, def->gravity_y, def->allow_sleep, def->warm_starting, def->continuous);
	*out = w;
	return 0;
}

void b2hip_world_destroy(b2hip_world* w)
{
	if (!w) return;
	b2o_world_destroy(w->o);
	free(w);
}

int b2hip_set_gravity(b2hip_world* w, float gx, float gy) { b2o_set_gravity(w->o, gx, gy); return 0; }

int b2hip_set_flags(b2hip_world* w, int allow_sleep, int warm_starting, int continuous, int sub_stepping)
{
	w->sub_stepping = sub_stepping;
	b2o_set_flags(w->o, allow_sleep, warm_starting, continuous);
	b2o_set_sub_stepping(w->o, sub_stepping);
	return 0;
}

int b2hip_create_body(b2hip_world* w, const b2hip_body_def* d)
{
	b2o_body_def o;
	memcpy(&o, d, sizeof(o)); /* identical field order */
	return b2o_create_body(w->o, &o);
}

int b2hip_create_fixture(b2hip_world* w, int body, const b2hip_fixture_def* d, const b2hip_shape* s)
{
	b2o_fixture_def fd;
	b2o_shape sh;
	memcpy(&fd, d, sizeof(fd));
	memcpy(&sh, s, sizeof(sh));
	w->fixtures++;
	return b2o_create_fixture(w->o, body, &fd, &sh);
}

int b2hip_create_revolute_joint(b2hip_world* w, const b2hip_revolute_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_revolute_joint(w->o, def->body_a, def->body_b, anchors, def->reference_angle, def->enable_limit,
		def->lower_angle, def->upper_angle, def->enable_motor, def->motor_speed, def->max_motor_torque, def->collide_connected);
}

int b2hip_create_distance_joint(b2hip_world* w, const b2hip_distance_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_distance_joint(w->o, def->body_a, def->body_b, anchors, def->length, def->frequency_hz, def->damping_ratio,
		def->collide_connected);
}

int b2hip_create_prismatic_joint(b2hip_world* w, const b2hip_prismatic_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_prismatic_joint(w->o, def->body_a, def->body_b, anchors, def->local_axis_a, def->reference_angle,
		def->enable_limit, def->lower_translation, def->upper_translation, def->enable_motor, def->motor_speed,
		def->max_motor_force, def->collide_connected);
}

int b2hip_create_weld_joint(b2hip_world* w, const b2hip_weld_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_weld_joint(w->o, def->body_a, def->body_b, anchors, def->reference_angle, def->frequency_hz,
		def->damping_ratio, def->collide_connected);
}

int b2hip_create_wheel_joint(b2hip_world* w, const b2hip_wheel_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_wheel_joint(w->o, def->body_a, def->body_b, anchors, def->local_axis_a, def->frequency_hz, def->damping_ratio,
		def->enable_motor, def->motor_speed, def->max_motor_torque, def->collide_connected);
}

int b2hip_create_rope_joint(b2hip_world* w, const b2hip_rope_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_rope_joint(w->o, def->body_a, def->body_b, anchors, def->max_length, def->collide_connected);
}

int b2hip_create_friction_joint(b2hip_world* w, const b2hip_friction_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	return b2o_create_friction_joint(w->o, def->body_a, def->body_b, anchors, def->max_force, def->max_torque, def->collide_connected);
}

int b2hip_create_motor_joint(b2hip_world* w, const b2hip_motor_joint_def* def)
{
	return b2o_create_motor_joint(w->o, def->body_a, def->body_b, def->linear_offset, def->angular_offset, def->max_force,
		def->max_torque, def->correction_factor, def->collide_connected);
}

int b2hip_create_pulley_joint(b2hip_world* w, const b2hip_pulley_joint_def* def)
{
	float anchors[4] = { def->local_anchor_a[0], def->local_anchor_a[1], def->local_anchor_b[0], def->local_anchor_b[1] };
	float grounds[4] = { def->ground_anchor_a[0], def->ground_anchor_a[1], def->ground_anchor_b[0], def->ground_anchor_b[1] };
	return b2o_create_pulley_joint(w->o, def->body_a, def->body_b, anchors, grounds, def->length_a, def->length_b, def->ratio,
		def->collide_connected);
}

int b2hip_create_mouse_joint(b2hip_world* w, const b2hip_mouse_joint_def* def)
{
	return b2o_create_mouse_joint(w->o, def->body_a, def->body_b, def->target[0], def->target[1], def->max_force, def->frequency_hz,
		def->damping_ratio, def->collide_connected);
}

int b2hip_create_gear_joint(b2hip_world* w, const b2hip_gear_joint_def* def)
{
	return b2o_create_gear_joint(w->o, def->joint1, def->joint2, def->ratio, def->collide_connected);
}

int b2hip_destroy_joint(b2hip_world* w, int joint)
{
	b2o_destroy_joint(w->o, joint);
	return 0;
}

int b2hip_joint_set_target(b2hip_world* w, int joint, float x, float y)
{
	b2o_joint_set_target(w->o, joint, x, y);
	return 0;
}

int b2hip_joint_set_offsets(b2hip_world* w, int joint, float lx, float ly, float angular)
{
	b2o_joint_set_offsets(w->o, joint, lx, ly, angular);
	return 0;
}

int b2hip_joint_set_motor(b2hip_world* w, int joint, int enable_motor, float motor_speed, float max_motor)
{
	b2o_joint_set_motor(w->o, joint, enable_motor, motor_speed, max_motor);
	return 0;
}

int b2hip_joint_set_limits(b2hip_world* w, int joint, int enable_limit, float lower, float upper)
{
	b2o_joint_set_limits(w->o, joint, enable_limit, lower, upper);
	return 0;
}

int b2hip_get_joint_reaction(b2hip_world* w, int joint, float inv_dt, float out4[4])
{
	b2o_get_joint_reaction(w->o, joint, inv_dt, out4);
	return 0;
}

int b2hip_body_count(const b2hip_world* w) { return b2o_body_count(w->o); }
int b2hip_fixture_count(const b2hip_world* w) { return w->fixtures; }

int b2hip_get_mass_data(const b2hip_world* w, int body, b2hip_mass_data* out)
{
	memset(out, 0, sizeof(*out));
	b2o_get_mass(w->o, body, &out->mass, &out->inertia, &out->local_center[0], &out->local_center[1]);
	return 0;
}

int b2hip_apply_force(b2hip_world* w, int body, float fx, float fy, float torque, int wake)
{
	b2o_apply_force(w->o, body, fx, fy, torque, wake);
	return 0;
}

int b2hip_set_velocity(b2hip_world* w, int body, float vx, float vy, float omega)
{
	b2o_set_velocity(w->o, body, vx, vy, omega);
	return 0;
}

int b2hip_step(b2hip_world* w, float dt, int vi, int pi)
{
	b2o_step(w->o, dt, vi, pi);
	/* (a spatially sharded world: a failed collective, or a TOI sub-step that created a contact - the merge of such contacts over
	 * the ranks is the product's, this shim does not restate it) */
	return b2o_spatial_failed(w->o) ? -4 : 0;
}

int b2hip_get_body_states(b2hip_world* w, int first, int count, b2hip_body_state* out)
{
	int n = b2o_body_count(w->o);
	float* tmp = (float*)malloc(sizeof(float) * 10 * (size_t)(n + 1));
	b2o_get_body_states(w->o, tmp);
	memcpy(out, tmp + 10 * first, sizeof(float) * 10 * (size_t)count);
	free(tmp);
	return 0;
}

int b2hip_contact_count(b2hip_world* w) { return b2o_contact_count(w->o); }

int b2hip_get_contacts(b2hip_world* w, int cap, b2hip_contact* out)
{
	return b2o_get_contacts(w->o, cap, (b2o_contact*)out); /* identical layout */
}

int b2hip_enable_contact_events(b2hip_world* w, int enable)
{
	b2o_enable_contact_events(w->o, enable);
	return 0;
}

int b2hip_get_contact_events(b2hip_world* w, int cap, b2hip_contact_event* out)
{
	return b2o_get_contact_events(w->o, cap, (b2o_contact_event*)out); /* identical layout */
}

int b2hip_step_begin(b2hip_world* w, float dt, int vi, int pi) { b2o_step_begin(w->o, dt, vi, pi); return 0; }
int b2hip_collide(b2hip_world* w) { b2o_phase_collide(w->o); return 0; }
int b2hip_solve(b2hip_world* w) { b2o_phase_solve(w->o); return 0; }
int b2hip_sync_fixtures(b2hip_world* w) { b2o_phase_sync_fixtures(w->o); return 0; }
int b2hip_find_new_contacts(b2hip_world* w) { b2o_phase_find_new_contacts(w->o); return 0; }
int b2hip_solve_toi(b2hip_world* w) { b2o_phase_solve_toi(w->o); return 0; }
int b2hip_step_end(b2hip_world* w) { b2o_step_end(w->o); return 0; }
int b2hip_set_shard(b2hip_world* w, int rank, int count)
{
	if (count < 1 || count > 8 || rank < 0 || rank >= count) return -1; /* B2HIP_ERR_INVALID: at most 8 ranks (the product's census arrays) */
	b2o_set_shard(w->o, rank, count);
	return 0;
}
/* spatial ownership: the same entry points as the product (include/b2hip.h) */
int b2hip_shard_spatial(b2hip_world* w, int rank, int count, const uint8_t* owners) { return b2o_shard_spatial(w->o, rank, count, owners); }
int b2hip_set_shard_gather(b2hip_world* w, b2hip_all_gather_fn fn, void* user) { b2o_set_shard_gather(w->o, fn, user); return 0; }
int b2hip_get_body_owners(b2hip_world* w, int cap, uint8_t* owners) { return b2o_get_body_owners(w->o, cap, owners); }
int b2hip_get_shard_stats(b2hip_world* w, b2hip_shard_stats* out)
{
	int32_t a[8];
	long long b[4];
	memset(out, 0, sizeof(*out));
	b2o_get_shard_stats(w->o, a, b);
	out->rank = a[0]; out->count = a[1]; out->owned_bodies = a[2]; out->owned_proxies = a[3]; out->owned_contacts = a[4];
	out->migrated_bodies = b[0]; out->resolutions = b[1]; out->bytes_received_last_step = b[2];
	return 0;
}
int b2hip_shard_tape(b2hip_world* w, int mode, b2hip_world* from) { (void)w; (void)mode; (void)from; return -4; }
int b2hip_get_own_body_states(b2hip_world* w, int cap, int32_t* ids, b2hip_body_state* out) { (void)w; (void)cap; (void)ids; (void)out; return -1; /* (this shim always exchanges full rows) */ }
int b2hip_shard_slab_words(b2hip_world* w, size_t* words_per_rank, int ranks)
{
	for (int r = 0; r < ranks; ++r) words_per_rank[r] = b2o_shard_slab_words(w->o, r);
	return 0;
}
int b2hip_shard_export(b2hip_world* w, void* slab, size_t words) { (void)words; b2o_shard_export(w->o, (int32_t*)slab); return 0; }
int b2hip_shard_import(b2hip_world* w, const void* all_slabs, size_t stride_words) { b2o_shard_import(w->o, (const int32_t*)all_slabs, stride_words); return 0; }

int b2hip_destroy_body(b2hip_world* w, int body) { b2o_destroy_body(w->o, body); return 0; }
int b2hip_destroy_fixture(b2hip_world* w, int fixture) { b2o_destroy_fixture(w->o, fixture); return 0; }
int b2hip_set_transform(b2hip_world* w, int body, float x, float y, float angle) { b2o_set_transform(w->o, body, x, y, angle); return 0; }
int b2hip_set_awake(b2hip_world* w, int body, int awake) { b2o_set_awake(w->o, body, awake); return 0; }
int b2hip_set_active(b2hip_world* w, int body, int active) { b2o_set_active(w->o, body, active); return 0; }
int b2hip_set_type(b2hip_world* w, int body, int type) { b2o_set_type(w->o, body, type); return 0; }
int b2hip_set_bullet(b2hip_world* w, int body, int bullet) { b2o_set_bullet(w->o, body, bullet); return 0; }
int b2hip_get_joint_limit_state(b2hip_world* w, int joint) { return b2o_get_joint_limit_state(w->o, joint); }
int b2hip_joint_set_param(b2hip_world* w, int joint, int param, float value) { return b2o_joint_set_param(w->o, joint, param, value) ? -1 : 0; }
int b2hip_shift_origin(b2hip_world* w, float x, float y) { b2o_shift_origin(w->o, x, y); return 0; }
int b2hip_set_body_damping(b2hip_world* w, int body, float l, float a, float g) { b2o_set_body_damping(w->o, body, l, a, g); return 0; }
int b2hip_set_fixed_rotation(b2hip_world* w, int body, int flag) { b2o_set_fixed_rotation(w->o, body, flag); return 0; }
int b2hip_set_sleeping_allowed(b2hip_world* w, int body, int flag) { b2o_set_sleeping_allowed(w->o, body, flag); return 0; }
int b2hip_set_mass_data(b2hip_world* w, int body, const b2hip_mass_data* md)
{
	if (md) b2o_set_mass_data(w->o, body, 1, md->mass, md->inertia, md->local_center[0], md->local_center[1]);
	else b2o_set_mass_data(w->o, body, 0, 0.0f, 0.0f, 0.0f, 0.0f);
	return 0;
}
int b2hip_fixture_set_material(b2hip_world* w, int fixture, float d, float f, float r) { b2o_fixture_set_material(w->o, fixture, d, f, r); return 0; }
int b2hip_apply_linear_impulse(b2hip_world* w, int body, float ix, float iy, float px, float py, int wake)
{
	b2o_apply_linear_impulse(w->o, body, ix, iy, px, py, 0, wake);
	return 0;
}
int b2hip_apply_linear_impulse_to_center(b2hip_world* w, int body, float ix, float iy, int wake)
{
	b2o_apply_linear_impulse(w->o, body, ix, iy, 0.0f, 0.0f, 1, wake);
	return 0;
}
int b2hip_apply_angular_impulse(b2hip_world* w, int body, float impulse, int wake) { b2o_apply_angular_impulse(w->o, body, impulse, wake); return 0; }
int b2hip_fixture_set_sensor(b2hip_world* w, int fixture, int is_sensor) { b2o_fixture_set_sensor(w->o, fixture, is_sensor); return 0; }
int b2hip_fixture_set_thick(b2hip_world* w, int fixture, int thick) { b2o_fixture_set_thick(w->o, fixture, thick); return 0; }
int b2hip_fixture_refilter(b2hip_world* w, int fixture) { b2o_fixture_refilter(w->o, fixture); return 0; }
int b2hip_fixture_set_filter(b2hip_world* w, int fixture, uint16_t category_bits, uint16_t mask_bits, int16_t group_index)
{
	b2o_fixture_set_filter(w->o, fixture, category_bits, mask_bits, group_index);
	return 0;
}
int b2hip_joint_set_spring(b2hip_world* w, int joint, float frequency_hz, float damping_ratio)
{
	b2o_joint_set_spring(w->o, joint, frequency_hz, damping_ratio);
	return 0;
}
int b2hip_body_is_destroyed(const b2hip_world* w, int body) { return b2o_body_is_destroyed(w->o, body); }
int b2hip_fixture_is_destroyed(const b2hip_world* w, int fixture) { return b2o_fixture_is_destroyed(w->o, fixture); }

int b2hip_set_contact_filter(b2hip_world* w, b2hip_should_collide_fn fn, void* user)
{
	b2o_set_contact_filter(w->o, (b2o_should_collide_fn)fn, user);
	return 0;
}

static int filter_batch_of_one(void* user, int fixture_a, int fixture_b)
{
	b2hip_world* w = (b2hip_world*)user;
	const int32_t pair[2] = { fixture_a, fixture_b };
	int32_t verdict = 1;
	w->filterBatch(w->filterBatchUser, 1, pair, &verdict);
	return verdict;
}

int b2hip_set_contact_filter_batch(b2hip_world* w, b2hip_should_collide_batch_fn fn, void* user)
{
	w->filterBatch = fn;
	w->filterBatchUser = user;
	b2o_set_contact_filter(w->o, fn ? filter_batch_of_one : NULL, w);
	return 0;
}

int b2hip_set_pre_solve_batch(b2hip_world* w, b2hip_pre_solve_batch_fn fn, void* user)
{
	b2o_set_pre_solve_batch(w->o, (b2o_pre_solve_batch_fn)fn, user); /* b2hip_pre_solve_record == b2o_pre_solve_record */
	return 0;
}

int b2hip_default_should_collide(b2hip_world* w, int fixture_a, int fixture_b)
{
	return b2o_default_should_collide(w->o, fixture_a, fixture_b);
}

int b2hip_set_pre_solve(b2hip_world* w, b2hip_pre_solve_fn fn, void* user)
{
	b2o_set_pre_solve(w->o, (b2o_pre_solve_fn)fn, user); /* b2hip_manifold == b2o_manifold */
	return 0;
}

int b2hip_get_toi_callbacks(b2hip_world* w, int cap, b2hip_toi_callback* out)
{
	return b2o_get_toi_callbacks(w->o, cap, (b2o_toi_callback*)out); /* same layout */
}

/* (a CPU world has nothing to read back: accepted, no effect) */
int b2hip_set_lazy_readback(b2hip_world* w, int enable)
{
	(void)w;
	(void)enable;
	return 0;
}

int b2hip_enable_post_solve(b2hip_world* w, int enable)
{
	b2o_enable_post_solve(w->o, enable);
	return 0;
}

int b2hip_get_post_solve(b2hip_world* w, int cap, b2hip_contact_impulse* out)
{
	return b2o_get_post_solve(w->o, cap, (b2o_contact_impulse*)out); /* identical layout */
}

int b2hip_get_island_labels(b2hip_world* w, int cap, int32_t* out)
{
	(void)cap;
	b2o_get_island_labels(w->o, out);
	return b2o_body_count(w->o);
}

int b2hip_get_fat_aabb(b2hip_world* w, int fixture, float out4[4])
{
	b2o_get_fat_aabb(w->o, fixture, out4);
	return 0;
}

int b2hip_get_fat_aabbs(b2hip_world* w, int first, int count, float* out4n)
{
	for (int i = 0; i < count; ++i) b2o_get_fat_aabb(w->o, first + i, out4n + 4 * i);
	return 0;
}

/* the oracle's solve order hook (b2o.h) on a world of this shim: what tests/test_gpu_solve_replay.py drives. No such entry
 * exists in the product. */
int b2o_shim_set_solve_order(b2hip_world* w, int count, const b2o_order_entry* entries, int body_count, const unsigned char* body_large,
	int joints_by_id)
{
	b2o_set_solve_order(w->o, count, entries, body_count, body_large, joints_by_id);
	return 0;
}

int b2o_shim_get_solve_order_errors(b2hip_world* w, int32_t errors[2])
{
	b2o_get_solve_order_errors(w->o, errors);
	return 0;
}

int b2o_shim_record_solve_order(b2hip_world* w, int enable) { b2o_record_solve_order(w->o, enable); return 0; }
int b2o_shim_get_recorded_solve_order(b2hip_world* w, int cap, b2o_order_entry* out) { return b2o_get_recorded_solve_order(w->o, cap, out); }

int b2hip_get_profile(b2hip_world* w, float ms[13])
{
	(void)w;
	memset(ms, 0, sizeof(float) * 13);
	return 0;
}
