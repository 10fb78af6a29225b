/* b2hip.h - C ABI of the MI355X-native b2World::Step() hot path (libb2hip.so).
 *
 * This is the drop-in boundary: plain C structs, pointers and sizes, no C++ and no torch types.
 * The host-side Box2D API mirror (box2d-mt_amd/host/Box2D/...) is a thin C++ layer that binds
 * exactly these entry points; INTEGRATION.md shows the binding a maintainer of the reference
 * would add inside b2World / b2Body.
 *
 * Reference interfaces replaced (all paths relative to the reference tree):
 *   b2hip_world_create / destroy     b2World::b2World, ~b2World            Box2D/Dynamics/b2World.cpp:446-520
 *   b2hip_create_body                b2World::CreateBody + b2Body::b2Body   b2World.cpp:548-582, b2Body.cpp:26-112
 *   b2hip_create_fixture             b2Body::CreateFixture, b2Fixture::Create/CreateProxies,
 *                                    b2Body::ResetMassData                  b2Body.cpp:182-226,310-385; b2Fixture.cpp:42-141
 *   b2hip_create_revolute_joint      b2World::CreateJoint (revolute)        b2World.cpp:672-760, Joints/b2RevoluteJoint.cpp:47-63
 *   b2hip_create_distance_joint      b2World::CreateJoint (distance)        b2World.cpp:672-760, Joints/b2DistanceJoint.cpp:51-63
 *   b2hip_create_prismatic_joint     b2World::CreateJoint (prismatic)       b2World.cpp:672-760, Joints/b2PrismaticJoint.cpp:98-128
 *   b2hip_create_weld_joint          b2World::CreateJoint (weld)            b2World.cpp:672-760, Joints/b2WeldJoint.cpp:46-56
 *   b2hip_create_wheel_joint         b2World::CreateJoint (wheel)           Joints/b2WheelJoint.cpp:47-77
 *   b2hip_create_rope_joint          b2World::CreateJoint (rope)            Joints/b2RopeJoint.cpp:34-46
 *   b2hip_create_friction_joint      b2World::CreateJoint (friction)        Joints/b2FrictionJoint.cpp:45-56
 *   b2hip_create_motor_joint         b2World::CreateJoint (motor)           Joints/b2MotorJoint.cpp:48-60
 *   b2hip_create_pulley_joint        b2World::CreateJoint (pulley)          Joints/b2PulleyJoint.cpp:62-79
 *   b2hip_create_mouse_joint         b2World::CreateJoint (mouse)           Joints/b2MouseJoint.cpp:36-55
 *   b2hip_create_gear_joint          b2World::CreateJoint (gear)            Joints/b2GearJoint.cpp:50-129
 *   b2hip_joint_set_target           b2MouseJoint::SetTarget                Joints/b2MouseJoint.cpp:57-64
 *   b2hip_joint_set_offsets          b2MotorJoint::SetLinearOffset / SetAngularOffset   Joints/b2MotorJoint.cpp:253-281
 *   b2hip_destroy_joint              b2World::DestroyJoint                  b2World.cpp:762-846
 *   b2hip_joint_set_motor            b2{Revolute,Prismatic,Wheel}Joint::EnableMotor / SetMotorSpeed / SetMaxMotor{Torque,Force}
 *                                                                           Joints/b2RevoluteJoint.cpp:418-452, b2PrismaticJoint.cpp:588-616
 *   b2hip_joint_set_limits           b2{Revolute,Prismatic}Joint::EnableLimit / SetLimits
 *                                                                           Joints/b2RevoluteJoint.cpp:459-500, b2PrismaticJoint.cpp:549-581
 *   b2hip_destroy_body / _fixture    b2World::DestroyBody, b2Body::DestroyFixture  b2World.cpp:585-670, b2Body.cpp:238-308
 *   b2hip_set_transform / _awake / _bullet, b2hip_apply_*_impulse           b2Body.cpp:451-473, 575-601; b2Body.h:690-718, 885-950
 *   b2hip_set_transforms / _awakes   b2Body::SetTransform / SetAwake for many bodies in one call (block H)   b2Body.cpp:451-473; b2Body.h:690-718
 *   b2hip_destroy_bodies / b2hip_set_actives   b2World::DestroyBody / b2Body::SetActive for many bodies in one call (block I)   b2World.cpp:585-670; b2Body.cpp:496-544
 *   b2hip_fixture_set_sensor / _thick / _filter, b2hip_fixture_refilter     b2Fixture.cpp:180-257
 *   b2hip_fixture_set_filters / _sensors / _thicks / _materials   b2Fixture::SetFilterData / SetSensor / SetThickShape / SetFriction ... for many fixtures in one call (block J)   b2Fixture.cpp:180-257; b2Fixture.h:306-334
 *   b2hip_set_types / _bullets / _fixed_rotations / _sleeping_alloweds / _body_dampings / _mass_datas, b2hip_reset_mass_datas
 *                                    b2Body::SetType / SetBullet / SetFixedRotation / SetSleepingAllowed / SetLinearDamping ... /
 *                                    SetMassData / ResetMassData for many bodies in one call (block K)   b2Body.cpp:116-175, 310-424, 546-565; b2Body.h:620-688
 *   b2hip_step                       b2World::Step                          b2World.cpp:1613-1710
 *   b2hip_collide                    b2World::Collide / b2ContactManager::Collide      b2World.cpp:1120-1141, b2ContactManager.cpp:177-230
 *   b2hip_solve                      b2World::Solve (islands + b2Island::Solve)        b2World.cpp:1166-1431, b2Island.cpp:184-396
 *   b2hip_sync_fixtures              b2World::SynchronizeFixtures                      b2World.cpp:1143-1164, b2ContactManager.cpp:315-364,441-452
 *   b2hip_find_new_contacts          b2World::FindNewContacts / b2BroadPhase::UpdatePairs / AddPair
 *                                                                                       b2World.cpp:1095-1118, b2BroadPhase.h:211-267, b2ContactManager.cpp:237-312,366-386
 *   b2hip_solve_toi                  b2World::SolveTOI                                 b2World.cpp:1026-1093, 851-1024
 *   b2hip_get_fat_aabbs              (served to) b2World::QueryAABB / RayCast          b2World.cpp:1740-1795, b2DynamicTree.h:168-287
 *   b2hip_get_body_states            b2Body::GetPosition/GetAngle/GetLinearVelocity/GetAngularVelocity/IsAwake  b2Body.h:516-700
 *   b2hip_enable/get_contact_events  b2ContactListener::BeginContact / EndContact     b2WorldCallbacks.h:88-104, b2ContactManager.cpp:420-438
 *   b2hip_set_pre_solve              b2ContactListener::PreSolve(Immediate)           b2WorldCallbacks.h:105-174, b2Contact.cpp:283-297
 *   b2hip_enable/get_post_solve      b2ContactListener::PostSolve(Immediate)          b2Island.cpp:532-570, b2ContactManager.cpp:454-470
 *   b2hip_set_contact_filter         b2ContactFilter::ShouldCollide                   b2WorldCallbacks.h:52-63, b2ContactManager.cpp:283-287
 *   b2hip_save / load_snapshot       (new: binary checkpoint; cf. b2World::Dump          b2World.cpp:2107-2164)
 *   b2hip_get_contacts               b2World::GetContactList + b2Contact::GetManifold  b2World.h:352-360, b2Contact.h:95-163
 *   b2hip_get_profile                b2World::GetProfile                    b2World.h:196-197, b2TimeStep.h:25-40
 *
 * Conventions: every function returns 0 on success and a negative b2hip_status on failure
 * (b2hip_last_error() gives the text); no exceptions cross the boundary; host buffers are owned by
 * the caller, device buffers by the world; all calls for one world come from one thread; work is
 * stream-ordered on the world's HIP stream and only the download / step calls block.
 * There is NO CPU fallback: if no HIP device is usable, b2hip_world_create fails.
 */
#ifndef B2HIP_H
#define B2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct b2hip_world b2hip_world;

typedef enum b2hip_status
{
	B2HIP_OK = 0,
	B2HIP_ERR_INVALID = -1,     /* bad argument / unknown id */
	B2HIP_ERR_HIP = -2,         /* a HIP runtime call failed */
	B2HIP_ERR_NO_DEVICE = -3,   /* no usable gfx950 device */
	B2HIP_ERR_UNSUPPORTED = -4, /* feature outside the device path */
	B2HIP_ERR_CAPACITY = -5     /* a device buffer overflowed and could not be regrown */
} b2hip_status;

enum { B2HIP_STATIC_BODY = 0, B2HIP_KINEMATIC_BODY = 1, B2HIP_DYNAMIC_BODY = 2 }; /* b2BodyType, b2Body.h:36-47 */
enum { B2HIP_SHAPE_CIRCLE = 0, B2HIP_SHAPE_EDGE = 1, B2HIP_SHAPE_POLYGON = 2,          /* b2Shape::Type, b2Shape.h:53-60 */
       /* ONE child of a b2ChainShape (b2ChainShape.h:32, GetChildEdge b2ChainShape.cpp:114-147): the record of an edge whose
        * ghost vertices are the child's neighbours. It collides, sweeps and ray-casts as that edge; its broad-phase AABB has no
        * radius (b2ChainShape.cpp:174-189). A chain fixture of n children is n consecutive fixtures of this type, created in
        * child order (the reference creates one proxy per child in that order, b2Fixture.cpp:126-141). */
       B2HIP_SHAPE_CHAIN = 3 };

typedef struct b2hip_world_def
{
	float gravity_x, gravity_y;
	int allow_sleep;      /* b2World::SetAllowSleeping      default 1 */
	int warm_starting;    /* b2World::SetWarmStarting       default 1 */
	int continuous;       /* b2World::SetContinuousPhysics  default 1 in the reference; continuous collision (TOI) runs on the device: b2hip_solve_toi */
	int sub_stepping;     /* b2World::SetSubStepping        default 0 ; a step call solves ONE TOI event and leaves the step open; the calls that
	                       *   follow run Collide and the next event, no island solve, until no event is left (b2World.cpp:1082-1086, 1668) */
	int auto_clear_forces;/* b2World::SetAutoClearForces    default 1 */
	int device;           /* HIP device ordinal, -1 = current */
} b2hip_world_def;

/* b2BodyDef (b2Body.h:52-129) */
typedef struct b2hip_body_def
{
	int type;
	float px, py, angle;
	float vx, vy, w;
	float linear_damping, angular_damping, gravity_scale;
	int allow_sleep, awake, fixed_rotation, bullet, active;
} b2hip_body_def;

/* A finished collision shape (what b2Shape::Clone would copy). Layout == device ShapeRec.
 *   circle : verts[0..1] = m_p, radius = m_radius
 *   edge   : verts[0..1] = m_vertex1, [2..3] = m_vertex2, [4..5] = m_vertex0, [6..7] = m_vertex3,
 *            count bit0 = m_hasVertex0, bit1 = m_hasVertex3, radius = b2_polygonRadius
 *   polygon: count, verts[2*count], normals[2*count], centroid, radius = b2_polygonRadius */
typedef struct b2hip_shape
{
	int32_t type;
	int32_t count;
	float radius;
	float pad;
	float centroid[2];
	float verts[16];
	float normals[16];
} b2hip_shape;

/* b2FixtureDef (b2Fixture.h:56-94) */
typedef struct b2hip_fixture_def
{
	float density, friction, restitution;
	uint16_t category_bits, mask_bits;
	int16_t group_index;
	int16_t pad;
	int is_sensor;
	int thick_shape;
} b2hip_fixture_def;

/* b2RevoluteJointDef (Joints/b2RevoluteJoint.h:35-85) */
typedef struct b2hip_revolute_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float reference_angle;
	int enable_limit;
	float lower_angle, upper_angle;
	int enable_motor;
	float motor_speed, max_motor_torque;
	int collide_connected;
} b2hip_revolute_joint_def;

/* b2DistanceJointDef (Joints/b2DistanceJoint.h:31-68): rigid rod when frequency_hz == 0, damped spring otherwise */
typedef struct b2hip_distance_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float length;
	float frequency_hz, damping_ratio;
	int collide_connected;
} b2hip_distance_joint_def;

/* b2PrismaticJointDef (Joints/b2PrismaticJoint.h:31-85): bodyB slides along local_axis_a of bodyA, no relative rotation */
typedef struct b2hip_prismatic_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float local_axis_a[2];          /* normalised at creation, like b2PrismaticJoint's constructor does */
	float reference_angle;
	int enable_limit;
	float lower_translation, upper_translation;
	int enable_motor;
	float motor_speed, max_motor_force;
	int collide_connected;
} b2hip_prismatic_joint_def;

/* b2WeldJointDef (Joints/b2WeldJoint.h:28-60): rigid when frequency_hz == 0, else a soft angular spring */
typedef struct b2hip_weld_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float reference_angle;
	float frequency_hz, damping_ratio;
	int collide_connected;
} b2hip_weld_joint_def;

/* b2WheelJointDef (Joints/b2WheelJoint.h:31-76): point-on-line along local_axis_a (used as given), suspension spring
 * along the axis (frequency_hz > 0) and a rotational motor */
typedef struct b2hip_wheel_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float local_axis_a[2];
	float frequency_hz, damping_ratio;
	int enable_motor;
	float motor_speed, max_motor_torque;
	int collide_connected;
} b2hip_wheel_joint_def;

/* b2RopeJointDef (Joints/b2RopeJoint.h:28-52): the anchors may not get further apart than max_length */
typedef struct b2hip_rope_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float max_length;
	int collide_connected;
} b2hip_rope_joint_def;

/* b2FrictionJointDef (Joints/b2FrictionJoint.h:26-51): top-down friction, force and torque capped */
typedef struct b2hip_friction_joint_def
{
	int body_a, body_b;
	float local_anchor_a[2], local_anchor_b[2];
	float max_force, max_torque;
	int collide_connected;
} b2hip_friction_joint_def;

/* b2PulleyJointDef (Joints/b2PulleyJoint.h:28-76): length_a + ratio * length_b stays constant; ground anchors in world space */
typedef struct b2hip_pulley_joint_def
{
	int body_a, body_b;
	float ground_anchor_a[2], ground_anchor_b[2];
	float local_anchor_a[2], local_anchor_b[2];
	float length_a, length_b;
	float ratio;
	int collide_connected;
} b2hip_pulley_joint_def;

/* b2MouseJointDef (Joints/b2MouseJoint.h:27-57): pulls the point of bodyB that lies at `target` (world) when the joint is
 * created towards wherever the target is moved; bodyA is only bookkeeping (the Testbed passes the ground body) */
typedef struct b2hip_mouse_joint_def
{
	int body_a, body_b;
	float target[2];
	float max_force;
	float frequency_hz, damping_ratio;
	int collide_connected;
} b2hip_mouse_joint_def;

/* b2GearJointDef (Joints/b2GearJoint.h:28-48): couples two existing revolute / prismatic joints (ids returned by their
 * create calls): coordinate1 + ratio * coordinate2 stays what it is at creation. The joint's bodies are the second bodies of the
 * two joints, as in the reference's constructor; the two joints must outlive the gear. */
typedef struct b2hip_gear_joint_def
{
	int joint1, joint2;
	float ratio;
	int collide_connected;
} b2hip_gear_joint_def;

/* b2MotorJointDef (Joints/b2MotorJoint.h:26-57): drives bodyB to linear_offset / angular_offset in bodyA's frame */
typedef struct b2hip_motor_joint_def
{
	int body_a, body_b;
	float linear_offset[2];
	float angular_offset;
	float max_force, max_torque;
	float correction_factor;
	int collide_connected;
} b2hip_motor_joint_def;

/* Host-visible body state after a step (40 bytes per body, one coalesced device->host copy). */
typedef struct b2hip_body_state
{
	float px, py;      /* b2Body::GetPosition  (m_xf.p)   */
	float angle;       /* b2Body::GetAngle     (m_sweep.a) */
	float vx, vy, w;   /* linear / angular velocity        */
	float cx, cy;      /* b2Body::GetWorldCenter (m_sweep.c) */
	uint32_t flags;    /* bit0-1 type, bit2 awake, bit3 autoSleep, bit4 bullet, bit5 fixedRotation, bit6 active */
	float sleep_time;
} b2hip_body_state;

#define B2HIP_BODY_AWAKE 0x4u

/* b2MassData + centre (b2Body::GetMass/GetInertia/GetLocalCenter) */
typedef struct b2hip_mass_data
{
	float mass, inertia;      /* inertia about the local origin, as b2Body::GetInertia returns it */
	float local_center[2];
	float inv_mass, inv_inertia;
} b2hip_mass_data;

/* One contact (b2Contact): fixture ids are the ids b2hip_create_fixture returned. */
typedef struct b2hip_contact
{
	int32_t fixture_a, fixture_b;
	int32_t body_a, body_b;
	uint32_t flags;            /* bit0 touching, bit1 enabled */
	int32_t manifold_type;     /* b2Manifold::Type */
	int32_t point_count;
	float local_normal[2];
	float local_point[2];
	float point_local[2][2];
	float normal_impulse[2];
	float tangent_impulse[2];
	uint32_t id_key[2];
	float friction, restitution;
	float tangent_speed;       /* b2Contact::GetTangentSpeed (b2Contact.h:157-160) */
} b2hip_contact;

/* Counters of the last step (device truth, read back with the body states). */
typedef struct b2hip_counters
{
	int32_t bodies, proxies, contacts, touching_contacts;
	int32_t islands, small_islands, large_islands;
	int32_t small_island_bodies, small_island_contacts, large_island_bodies, large_island_contacts;
	int32_t colors, moved_proxies, new_contacts, destroyed_contacts;
	int32_t solver_chunks;
	int32_t pos_iterations_large;
	int32_t overflow_flags;
	int32_t toi_events;              /* TOI sub-steps solved in the last step (b2World::StepSolveTOI calls) */
	int32_t toi_calls;               /* b2TimeOfImpact evaluations in the last step */
	int32_t toi_pending_first_pass;  /* contacts whose first-pass time of impact was < 1 */
	int32_t toi_serial_fallbacks;    /* steps (since creation) whose parallel TOI chains were redone by the serial event loop */
	/* block partition of the large islands (one workgroup solves one block with its bodies in LDS) */
	int32_t blocks;                  /* blocks of the current partition */
	int32_t cut_constraints;         /* constraints between bodies of two blocks in the last step */
	int32_t block_max_rows;          /* most constraints owned by one block in the last step */
	int32_t partitions;              /* partitions made since the world was created */
	int32_t block_solver_steps;      /* steps whose large islands were solved by the block solver */
	int32_t free_islands;            /* one-body islands without contact or joint in the last step (stepped without the island solver) */
	int32_t sweep_solver_steps;      /* steps whose (jointed / hub) large islands took the one-launch-per-sweep block kernel */
	/* hub bodies (more contacts than can be coloured): their constraints are swept in order by one wave (k_large_hub) */
	int32_t hub_constraints;         /* hub constraints in the last step */
	int32_t hub_fixpoint_rounds;     /* rounds of the fixed-point form of that sweep in the last step (all sweeps) */
	int32_t hub_serial_chunks;       /* chunks of 64 hub constraints swept lane after lane instead */
	int32_t toi_chain_contacts;      /* contacts (since creation) the parallel TOI chains left for their close-out to create in event order */
	int32_t toi_pre_solve_reruns;    /* runs of the TOI phase (since creation) repeated because a PreSolve changed its contact inside a sub-step */
	int32_t solver_recoveries;       /* large-island solves (since creation) run a second time, launch by launch, because a wait between the
	                                    workgroups of a resident / data-flow solver kernel timed out, or whose colouring ran out of colours (such constraints are
	                                    swept in order) or of rounds (finished grid-wide); the step itself succeeds (B2HIP_NO_RECOVER=1: it fails as before) */
} b2hip_counters;

const char* b2hip_last_error(void);
const char* b2hip_version(void);

int b2hip_world_create(const b2hip_world_def* def, b2hip_world** out);
void b2hip_world_destroy(b2hip_world* w);

int b2hip_set_gravity(b2hip_world* w, float gx, float gy);
/* b2World::ShiftOrigin (b2World.cpp:1862-1887): bodies, broad-phase boxes and the world-space anchors of mouse and pulley
 * joints move by -(x, y); between steps only. */
int b2hip_shift_origin(b2hip_world* w, float x, float y);
int b2hip_set_flags(b2hip_world* w, int allow_sleep, int warm_starting, int continuous, int sub_stepping);

/* Returns the new body / fixture / joint id (>= 0) or a negative status. */
int b2hip_create_body(b2hip_world* w, const b2hip_body_def* def);
int b2hip_create_fixture(b2hip_world* w, int body, const b2hip_fixture_def* def, const b2hip_shape* shape);
int b2hip_create_revolute_joint(b2hip_world* w, const b2hip_revolute_joint_def* def);
int b2hip_create_distance_joint(b2hip_world* w, const b2hip_distance_joint_def* def);
int b2hip_create_prismatic_joint(b2hip_world* w, const b2hip_prismatic_joint_def* def);
int b2hip_create_weld_joint(b2hip_world* w, const b2hip_weld_joint_def* def);
int b2hip_create_wheel_joint(b2hip_world* w, const b2hip_wheel_joint_def* def);
int b2hip_create_rope_joint(b2hip_world* w, const b2hip_rope_joint_def* def);
int b2hip_create_friction_joint(b2hip_world* w, const b2hip_friction_joint_def* def);
int b2hip_create_motor_joint(b2hip_world* w, const b2hip_motor_joint_def* def);
int b2hip_create_pulley_joint(b2hip_world* w, const b2hip_pulley_joint_def* def);
int b2hip_create_mouse_joint(b2hip_world* w, const b2hip_mouse_joint_def* def);
int b2hip_create_gear_joint(b2hip_world* w, const b2hip_gear_joint_def* def);
/* b2MouseJoint::SetTarget (b2MouseJoint.cpp:57-64): wakes bodyB when the target moves */
int b2hip_joint_set_target(b2hip_world* w, int joint, float x, float y);
/* b2MotorJoint::SetLinearOffset + SetAngularOffset (b2MotorJoint.cpp:253-281): wakes both bodies when something changes */
int b2hip_joint_set_offsets(b2hip_world* w, int joint, float linear_x, float linear_y, float angular);
/* b2World::DestroyJoint (b2World.cpp:762-846): wakes both bodies; contacts between them are filtered again if the joint
 * kept them from colliding. Joint ids are never reused (the id of a destroyed joint stays invalid). Destroy a gear joint
 * before the joints it couples. */
int b2hip_destroy_joint(b2hip_world* w, int joint);
/* Revolute / prismatic / wheel (motor only) joints between steps: EnableMotor + SetMotorSpeed + SetMaxMotorTorque|Force in one call, and
 * EnableLimit + SetLimits in one call. Like the reference's setters, a call that changes something wakes both bodies and
 * (limits) restarts the limit impulse from zero; a call that changes nothing does nothing. */
int b2hip_joint_set_motor(b2hip_world* w, int joint, int enable_motor, float motor_speed, float max_motor);
int b2hip_joint_set_limits(b2hip_world* w, int joint, int enable_limit, float lower, float upper);
/* b2Joint::GetReactionForce / GetReactionTorque(inv_dt) and the motor's share (b2RevoluteJoint::GetMotorTorque,
 * b2PrismaticJoint::GetMotorForce, b2WheelJoint::GetMotorTorque) after the last step, from the joint's accumulated impulses
 * (b2Joint.h:129-133; per type: b2RevoluteJoint.cpp:439-456, b2PrismaticJoint.cpp:502-510,618-621, ...).
 * out4 = force.x, force.y, torque, motor. One small device read per call (between steps). */
int b2hip_get_joint_reaction(b2hip_world* w, int joint, float inv_dt, float out4[4]);
/* b2RopeJoint::GetLimitState (b2RopeJoint.h:84; also the limit state of revolute / prismatic joints): 0 inactive, 1 at lower,
 * 2 at upper, 3 equal limits (b2LimitState, b2Joint.h:58-64) as the last step's solver left it; negative = error code. */
int b2hip_get_joint_limit_state(b2hip_world* w, int joint);

/* ---- Life cycle and mutators between steps (all refused inside a step, like the reference's locked world) -------------------
 * Ids are never reused: a destroyed body / fixture keeps its id (every getter reports it as destroyed), so ids handed
 * out earlier stay valid. Edits that touch the contact array (destroys, TOI candidacy, re-filtering) are applied in call
 * order by one device pass at the start of the next step, or when the contacts are read.
 *
 * b2World::DestroyBody (b2World.cpp:585-670): its joints (b2hip_destroy_joint each, newest first), then its contacts
 * (newest first; a touching one reports its EndContact), then its fixtures and their broad-phase proxies (newest first:
 * proxy ids are freed and reused exactly as the reference's tree does), then the body leaves m_nonStaticBodies (the last
 * non-static body takes its slot, which is the order islands are seeded in). */
int b2hip_destroy_body(b2hip_world* w, int body);
/* b2Body::DestroyFixture (b2Body.cpp:238-308): the fixture's contacts, its proxy, then ResetMassData */
int b2hip_destroy_fixture(b2hip_world* w, int fixture);
/* b2Body::SetTransform (b2Body.cpp:451-473): pose and sweep (origin included) are set, every fixture is synchronised with
 * zero displacement (a proxy that leaves its fat AABB is re-inserted and buffered as moved) */
int b2hip_set_transform(b2hip_world* w, int body, float x, float y, float angle);
/* b2Body::SetAwake (b2Body.h:690-718): true restarts the sleep timer; false also zeroes velocities and forces */
int b2hip_set_awake(b2hip_world* w, int body, int awake);
/* b2Body::SetActive (b2Body.cpp:496-544): an inactive body keeps its fixtures but has no broad-phase proxies and no contacts
 * (they are destroyed in its contact-list order) and is skipped by the island build, joints to it included; activating it
 * creates the proxies again, newest fixture first, with fresh proxy ids - contacts follow with the next pair update. */
int b2hip_set_active(b2hip_world* w, int body, int active);
/* b2Body::SetType (b2Body.cpp:118-188): type = B2HIP_STATIC_BODY / KINEMATIC / DYNAMIC. Mass data are recomputed, a body
 * that becomes static stops and its proxies are synchronised, the body moves between the world's static and non-static
 * lists (the island seed order follows), wakes, loses its forces and ALL its contacts; its proxies are touched so that
 * the next pair update forms the contacts its new type allows. */
int b2hip_set_type(b2hip_world* w, int body, int type);
/* b2Body::SetBullet (b2Body.cpp:575-601) + b2ContactManager::RecalculateToiCandidacy (b2ContactManager.cpp:566-640) */
int b2hip_set_bullet(b2hip_world* w, int body, int bullet);
/* b2Body::ApplyLinearImpulse / ApplyLinearImpulseToCenter (point = world centre) / ApplyAngularImpulse (b2Body.h:885-950) */
int b2hip_apply_linear_impulse(b2hip_world* w, int body, float ix, float iy, float px, float py, int wake);
int b2hip_apply_linear_impulse_to_center(b2hip_world* w, int body, float ix, float iy, int wake);
int b2hip_apply_angular_impulse(b2hip_world* w, int body, float impulse, int wake);
/* b2Fixture::SetSensor (b2Fixture.cpp:222-239: wakes the body, re-evaluates TOI candidacy), SetThickShape (:241-257),
 * SetFilterData + Refilter (:180-220: contacts of the fixture are filtered again by the next Collide, the proxy is
 * touched so that new pairs can form) */
int b2hip_fixture_set_sensor(b2hip_world* w, int fixture, int is_sensor);
int b2hip_fixture_set_thick(b2hip_world* w, int fixture, int thick_shape);
int b2hip_fixture_set_filter(b2hip_world* w, int fixture, uint16_t category_bits, uint16_t mask_bits, int16_t group_index);
int b2hip_fixture_refilter(b2hip_world* w, int fixture);
/* b2Fixture::SetDensity / SetFriction / SetRestitution (b2Fixture.h:306-334): the density is read by the next ResetMassData
 * (b2hip_set_mass_data(w, body, NULL)), friction and restitution by contacts created from now on. */
int b2hip_fixture_set_material(b2hip_world* w, int fixture, float density, float friction, float restitution);
/* b2Body::SetLinearDamping / SetAngularDamping / SetGravityScale (b2Body.h:620-648) */
int b2hip_set_body_damping(b2hip_world* w, int body, float linear_damping, float angular_damping, float gravity_scale);
/* b2Body::SetFixedRotation (b2Body.cpp:546-565) and b2Body::SetSleepingAllowed (b2Body.h:674-688) */
int b2hip_set_fixed_rotation(b2hip_world* w, int body, int flag);
int b2hip_set_sleeping_allowed(b2hip_world* w, int body, int flag);
/* b2WheelJoint / b2DistanceJoint / b2WeldJoint / b2MouseJoint ::SetFrequency / SetSpringFrequencyHz + SetDampingRatio
 * (e.g. b2WheelJoint.h:125-131): plain member writes, nobody is woken */
int b2hip_joint_set_spring(b2hip_world* w, int joint, float frequency_hz, float damping_ratio);
/* The plain scalar setters of the joint classes (assignments in the reference, no wake-up): b2DistanceJoint::SetLength,
 * b2RopeJoint::SetMaxLength (LENGTH); b2FrictionJoint / b2MotorJoint / b2MouseJoint::SetMaxForce (MAX_FORCE);
 * b2FrictionJoint / b2MotorJoint::SetMaxTorque (MAX_TORQUE); b2GearJoint::SetRatio (RATIO);
 * b2MotorJoint::SetCorrectionFactor (CORRECTION_FACTOR). A parameter the joint's type does not have: B2HIP_ERR_INVALID. */
enum { B2HIP_JOINT_LENGTH = 0, B2HIP_JOINT_MAX_FORCE = 1, B2HIP_JOINT_MAX_TORQUE = 2, B2HIP_JOINT_RATIO = 3, B2HIP_JOINT_CORRECTION_FACTOR = 4 };
int b2hip_joint_set_param(b2hip_world* w, int joint, int param, float value);
/* 1 if the id names a body / fixture that has been destroyed */
int b2hip_body_is_destroyed(const b2hip_world* w, int body);
int b2hip_fixture_is_destroyed(const b2hip_world* w, int fixture);

int b2hip_body_count(const b2hip_world* w);
int b2hip_fixture_count(const b2hip_world* w);
int b2hip_get_mass_data(const b2hip_world* w, int body, b2hip_mass_data* out);
/* b2Body::SetMassData (b2Body.cpp:387-424: dynamic bodies only; `inertia` about the body origin); mass_data == NULL:
 * b2Body::ResetMassData (b2Body.cpp:310-385: from the fixtures' shapes and densities). */
int b2hip_set_mass_data(b2hip_world* w, int body, const b2hip_mass_data* mass_data);

/* Force / impulse staging between steps (b2Body::ApplyForceToCenter, ApplyTorque, SetLinearVelocity ...). */
int b2hip_apply_force(b2hip_world* w, int body, float fx, float fy, float torque, int wake);
int b2hip_set_velocity(b2hip_world* w, int body, float vx, float vy, float omega);

/* One full b2World::Step on the device, then the body-state read-back. Blocking. */
int b2hip_step(b2hip_world* w, float dt, int velocity_iterations, int position_iterations);

/* The phases of Step as separate entry points (each blocks until its kernels are done) so that every
 * phase can be parity-tested and profiled alone. b2hip_step == begin, [find_new_contacts], collide,
 * solve, sync_fixtures, find_new_contacts, end. */
int b2hip_step_begin(b2hip_world* w, float dt, int velocity_iterations, int position_iterations);
int b2hip_collide(b2hip_world* w);
int b2hip_solve(b2hip_world* w);
int b2hip_sync_fixtures(b2hip_world* w);
int b2hip_find_new_contacts(b2hip_world* w);
/* b2World::SolveTOI (b2World.cpp:1026-1093): continuous collision, after the end-of-step pair update.
 * No-op unless the world was created / flagged with continuous = 1. */
int b2hip_solve_toi(b2hip_world* w);
int b2hip_step_end(b2hip_world* w);

/* Host mirror of the last read-back; valid until the next step. */
int b2hip_get_body_states(b2hip_world* w, int first, int count, b2hip_body_state* out);
int b2hip_contact_count(b2hip_world* w);
int b2hip_get_contacts(b2hip_world* w, int cap, b2hip_contact* out);

/* Contact events: the BeginContact / EndContact half of b2ContactListener (b2WorldCallbacks.h:88-174; generation sites
 * b2Contact.cpp:253-297, b2ContactManager.cpp:104-107; delivery order b2ContactManager.cpp:420-438). When enabled, every
 * step ends with the list of contacts whose touching state changed since the host was last told: all begins in
 * proxy-id-pair order, then all ends in proxy-id-pair order (the order in which the reference delivers its deferred
 * callbacks). One net event per contact and step: a contact that begins AND ends inside one step (continuous-collision
 * sub-steps) produces none, where the reference may call both. `contact_index` = index into b2hip_get_contacts of the
 * same step, or -1 when the contact was destroyed (its end event). Sensors report like any contact. */
typedef struct b2hip_contact_event
{
	int32_t fixture_a, fixture_b;
	int32_t kind;              /* 0 = begin, 1 = end */
	int32_t contact_index;
} b2hip_contact_event;
int b2hip_enable_contact_events(b2hip_world* w, int enable);
/* returns the number of events of the last step (negative on error); at most `cap` are written */
int b2hip_get_contact_events(b2hip_world* w, int cap, b2hip_contact_event* out);
/* ---- The other half of b2ContactListener, and b2ContactFilter: user code in the middle of a step ----------------------------
 * The physics runs on the device, user code on the host: each of these is a plain C callback the step calls on the
 * stepping thread at the point where the reference calls the listener / filter, between two device phases.
 * Installing one costs a device -> host round trip per step at that point (and only then).
 *
 * b2ContactFilter::ShouldCollide (b2WorldCallbacks.h:52-63; call sites b2ContactManager.cpp:283-287 AddPair, :195-203 the
 * re-filter of flagged contacts in Collide): called for every NEW candidate pair that has passed the body rules (same
 * body, existing contact, joints, one dynamic body) and for every contact flagged for re-filtering; return 0 to refuse.
 * An installed filter REPLACES the built-in category / mask / group rule, as a user b2ContactFilter replaces the default
 * one (call b2hip_default_should_collide from it to keep that rule). Not consulted for contacts created inside a
 * continuous-collision sub-step (those are made on the device with the built-in rule). */
typedef int (*b2hip_should_collide_fn)(void* user, int fixture_a, int fixture_b);
int b2hip_set_contact_filter(b2hip_world* w, b2hip_should_collide_fn fn, void* user);
/* ... or all pairs of one decision point in one call (fixture_pairs = count x {a, b}, verdict[i] = 0 refuses pair i): the
 * form for a caller that asks b2ContactFilter::ShouldCollide(fA, fB, threadId) from several threads (b2WorldCallbacks.h:57-62). */
typedef void (*b2hip_should_collide_batch_fn)(void* user, int count, const int32_t* fixture_pairs, int32_t* verdict);
int b2hip_set_contact_filter_batch(b2hip_world* w, b2hip_should_collide_batch_fn fn, void* user);
/* the built-in rule: b2ContactFilter::ShouldCollide (b2WorldCallbacks.cpp:24-38) on the fixtures' filter data */
int b2hip_default_should_collide(b2hip_world* w, int fixture_a, int fixture_b);

/* b2Manifold as the listener sees it (b2Collision.h:93-107) */
typedef struct b2hip_manifold
{
	int32_t type, point_count;
	float local_normal[2], local_point[2];
	float point_local[2][2];
	float normal_impulse[2], tangent_impulse[2];
	uint32_t id_key[2];
} b2hip_manifold;

/* b2ContactListener::PreSolve (b2WorldCallbacks.h:88-174; generation site b2Contact.cpp:283-297, delivery
 * b2ContactManager.cpp:431-434): after Collide, before the islands are built, once per touching non-sensor contact that
 * was updated in this step, in proxy-id-pair order, with the manifold of the previous step. Return 0 to disable the
 * contact for this step (b2Contact::SetEnabled(false): it is left out of the islands; the next Collide enables it again).
 * `contact_index` indexes b2hip_get_contacts. Contacts updated inside continuous-collision sub-steps are not reported. */
/* `material` (in / out): the contact's mixed friction and restitution (b2Contact.h:40-50) and its tangent speed, as
 * b2Contact::SetFriction / SetRestitution / SetTangentSpeed (b2Contact.h:129-160) may change them from inside the callback;
 * what the callback leaves there stays with the contact (this step's solver and every later one, until it is set again). */
typedef struct b2hip_contact_material
{
	float friction, restitution, tangent_speed;
} b2hip_contact_material;
typedef int (*b2hip_pre_solve_fn)(void* user, int contact_index, int fixture_a, int fixture_b,
	const b2hip_manifold* old_manifold, const b2hip_manifold* manifold, b2hip_contact_material* material);
int b2hip_set_pre_solve(b2hip_world* w, b2hip_pre_solve_fn fn, void* user);

/* The same delivery as ONE call per step with all records (in the deferred order): the form a caller uses that wants to run
 * b2ContactListener::PreSolveImmediate on the worker threads of its b2TaskExecutor, as the reference does during Collide
 * (b2WorldCallbacks.h:135-173, b2Contact.cpp:283-297), and the deferred PreSolve afterwards in order. The callee fills
 * `enabled` (in: 1) and `material` (in: the contact's values) of every record. Installing a batch function replaces the
 * per-record one. */
typedef struct b2hip_pre_solve_record
{
	int32_t contact_index, fixture_a, fixture_b;
	int32_t enabled;
	b2hip_manifold old_manifold, manifold;
	b2hip_contact_material material;
} b2hip_pre_solve_record;
typedef void (*b2hip_pre_solve_batch_fn)(void* user, int count, b2hip_pre_solve_record* records);
int b2hip_set_pre_solve_batch(b2hip_world* w, b2hip_pre_solve_batch_fn fn, void* user);

/* The listener calls the reference makes from INSIDE its TOI sub-steps (b2World::SolveTOI -> StepSolveTOI, b2World.cpp:866,946:
 * contact->Update(listener) on the TOI contact and on every contact of the two bodies it visits; b2Island::SolveTOI ->
 * Report, b2Island.cpp:527): the last step's calls in the reference's call order - event after event, inside an event the
 * TOI contact's Update, the visited contacts' Updates in walk order, then PostSolve for the sub-step's island in island
 * order. They come after the Collide / Solve callbacks of the step (b2hip_get_contact_events, PreSolve, b2hip_get_post_solve).
 * One record per call site; `kind` says which callbacks it stands for (an Update can be BeginContact + PreSolve at once):
 *   bit0 BeginContact, bit1 EndContact, bit2 PreSolve(old_manifold), bit3 PostSolve (manifold.normal_impulse / tangent_impulse
 *   = the sub-step solver's impulses, manifold.point_count = its point count).
 * Recorded while begin / end events, a PreSolve function or PostSolve records are switched on (each kind only if its
 * callback is), and the TOI phase then runs through the serial event loop (the order IS the serial order).
 * PreSolve is the exception, because what it does to its contact - a zero return (b2Contact::SetEnabled(false)), an edited
 * material - changes the sub-step that called it (b2World.cpp:873-881, 948-954: a contact switched off keeps the sweeps of
 * its bodies and stays out of the sub-step's island): the function installed with b2hip_set_pre_solve /
 * b2hip_set_pre_solve_batch (one record per call) is called BY THE STEP for every such Update, in the reference's order,
 * each exactly once, and its answer acts where the reference's does. The device's event loop is one kernel: an answer that
 * changes its contact sends the phase back to its snapshot for another run with the answers so far (one extra run per
 * changing answer, b2hip_counters.toi_pre_solve_reruns). World edits made from such a call reach the device before the next
 * step; a call that edits the world AND changes its contact is refused (B2HIP_ERR_INVALID). bit2 therefore never shows in
 * the records read here. */
typedef struct b2hip_toi_callback
{
	int32_t kind;
	int32_t contact_index, fixture_a, fixture_b;
	b2hip_manifold old_manifold, manifold;
	b2hip_contact_material material;
} b2hip_toi_callback;
int b2hip_get_toi_callbacks(b2hip_world* w, int cap, b2hip_toi_callback* out);

/* b2ContactListener::PostSolve (generation b2Island.cpp:532-570, delivery b2ContactManager.cpp:454-470): the impulses the
 * solver ended with, one record per contact constraint of every island solved in the last step, in proxy-id-pair order.
 * `count` is the solver's point count (1 when the block solver's conditioning guard dropped the second point,
 * b2ContactSolver.cpp:230-247). The sub-step islands of continuous collision are not reported. */
typedef struct b2hip_contact_impulse
{
	int32_t fixture_a, fixture_b;
	int32_t contact_index;
	int32_t count;
	float normal_impulses[2];
	float tangent_impulses[2];
} b2hip_contact_impulse;
int b2hip_enable_post_solve(b2hip_world* w, int enable);
/* returns the number of records of the last step (negative on error); at most `cap` are written */
int b2hip_get_post_solve(b2hip_world* w, int cap, b2hip_contact_impulse* out);

/* ---- One world over the GPUs of a node, sharded by island ----------------------------------------------
 * Every rank builds the SAME world with the same calls and steps it; Collide, the island build, the broad-phase and the TOI
 * phase run replicated, b2Island::Solve runs for the islands a rank owns (b2World.cpp:1236-1241: islands share only static
 * bodies), and after the solve the ranks all-gather the records of what they own (a "slab" per rank: 52 B per body, 20 B per
 * contact, 24 B per joint of ITS islands; every record carries its id).
 *
 * (1) Inside the library, RCCL over xGMI on the world's own stream - no host synchronisation, nothing to call per step:
 *       rank 0: b2hip_shard_unique_id(id)  ->  hand the 128 bytes to every rank (any means: a file, MPI, torch.distributed)
 *       every rank: b2hip_shard_connect(world, id, rank, count)   (one GPU per rank, at most 8 ranks; librccl is opened here)
 *       ... b2hip_step as usual (the drop-in b2World::Step needs no change).
 * (2) With a collective of the caller's (the CPU tests use gloo through torch.distributed), per step, inside
 *     b2hip_step_begin .. b2hip_step_end, between b2hip_solve and b2hip_sync_fixtures:
 *       b2hip_set_shard(world, rank, count) once;
 *       b2hip_shard_slab_words(world, words[count], count): the slab sizes of ALL ranks (every rank knows them: the island
 *         build is replicated) -> stride = max; b2hip_shard_export(slab, stride): this rank's slab (memory the library can
 *         address: DEVICE memory for libb2hip); all-gather of `stride` int32 per rank;
 *         b2hip_shard_import(all_slabs, stride): the other ranks' results enter the world.
 * box2d-mt_amd/python/sharding.py (ShardedWorld) drives either. With one rank (the default) nothing changes. */
int b2hip_set_shard(b2hip_world* w, int rank, int count);
int b2hip_shard_slab_words(b2hip_world* w, size_t* words_per_rank, int ranks);
int b2hip_shard_export(b2hip_world* w, void* slab, size_t words);
int b2hip_shard_import(b2hip_world* w, const void* all_slabs, size_t stride_words);
int b2hip_shard_unique_id(void* id128);
int b2hip_shard_connect(b2hip_world* w, const void* id128, int rank, int count);
/* bytes the last step's all-gather moved into this rank (count x stride x 4) */
int b2hip_shard_exchange_bytes(b2hip_world* w, size_t* bytes);

/* ---- ... or by SPATIAL OWNERSHIP (round 4; SURVEY.md section 8e: "persistent ownership by spatial cell -> GPU"; the reference
 * partitions the same phases over its threads: b2CollideTask b2World.cpp:100, b2BroadphaseSyncFixturesTask :120,
 * b2BroadphaseFindNewContactsTask :142, islands :1236-1241) -------------------------------------------------------------------
 * Every rank builds the SAME world with the same calls; ids mean the same everywhere. Every non-static body has one OWNER.
 * A rank evaluates manifolds, builds islands, solves, synchronises fixtures, searches pairs and runs TOI events for the
 * bodies it owns only; what it keeps of the others is the replicated tables of section 8e (pose / velocity rows, fat AABBs)
 * and the structure of the contact array (which contacts exist, in which order - so that every order the reference's
 * results depend on stays the unsharded world's). Per step it receives: the rows and fat AABBs of the bodies the others
 * moved (after Solve and after SolveTOI) and the new pairs the others found; when a new contact joins bodies of different
 * owners, the smaller side's connected component migrates (contact and joint content is shipped once).
 * Results are bit-identical to the unsharded world in every mode whose island solve is (reference-order tier, exact-order
 * mode); large islands in the coloured order stay in their parity class (the block partition is a rank's own).
 *
 *   b2hip_shard_spatial(world, rank, count, owners): between steps, once the bodies exist. owners[b2hip_body_count] = owning
 *     rank per body (static bodies: ignored), or NULL: strips of equal body count along x. The same on every rank.
 *     Bodies created later fall into the strip of their x. Contacts and joints that join bodies of different owners are
 *     resolved at the next step (the component goes to the rank that owns most of it).
 *   the collective: b2hip_shard_connect (RCCL, as above), or b2hip_set_shard_gather: `fn(user, send, bytes, recv)` must
 *     place every rank's `bytes` bytes at recv + rank * bytes on every rank (an all-gather over HOST memory; gloo in the
 *     CPU tests, a thread barrier in the one-process GPU tests) and return 0.
 *   b2hip_get_shard_stats: what this rank owns and what the exchanges moved.
 * Not supported in a spatially sharded world (refused with B2HIP_ERR_UNSUPPORTED): contact listeners / filters, sub-stepping. */
typedef int (*b2hip_all_gather_fn)(void* user, const void* send, size_t bytes, void* recv);
typedef struct b2hip_shard_stats
{
	int32_t rank, count;
	int32_t owned_bodies, owned_proxies;     /* non-static bodies this rank owns, and their proxies */
	int32_t owned_contacts;                  /* contacts whose content this rank maintains (the others are structure only) */
	int32_t islands_solved;                  /* islands of the last step (this rank's) */
	int32_t constraint_rows;                 /* solid contacts in this rank's islands in the last step */
	int64_t migrated_bodies;                 /* bodies that changed owner since the world was sharded */
	int64_t resolutions;                     /* times a straddling contact / joint made components merge */
	int64_t bytes_received_last_step;        /* all exchanges of the last step */
	int64_t pairs_sent;                      /* new pairs this rank found and sent, since the world was sharded */
	int64_t toi_redos;                       /* TOI phases run again because an event reached over an ownership boundary */
} b2hip_shard_stats;
int b2hip_shard_spatial(b2hip_world* w, int rank, int count, const uint8_t* owners);
int b2hip_set_shard_gather(b2hip_world* w, b2hip_all_gather_fn fn, void* user);
int b2hip_get_shard_stats(b2hip_world* w, b2hip_shard_stats* out);
/* Measurement hook (tools/gpu_spatial_share.py): mode 1 - keep the result of every collective of `w` in device memory; mode 2 -
 * `w` takes its collectives' results from the tape of `from` (a world of the same rank that recorded the same run) instead
 * of running a collective: one rank of a sharded world stepped alone on one GPU; mode 0 - off. */
int b2hip_shard_tape(b2hip_world* w, int mode, b2hip_world* from);
/* Lean exchange (the default): the rows of the bodies THIS rank owns as the last step left them, packed - what the step
 * brought to the host (1 / N of the table crosses PCIe; the table of all rows stays on the device until b2hip_get_body_states
 * asks for it, as with b2hip_set_lazy_readback). ids[k] = body, out[k] = its state; returns the number of rows (at most cap). */
int b2hip_get_own_body_states(b2hip_world* w, int cap, int32_t* ids, b2hip_body_state* out);
/* the owner table as it stands (owners[b2hip_body_count]); between steps */
int b2hip_get_body_owners(b2hip_world* w, int cap, uint8_t* owners);

/* Island label per body for the last step: -1 = not solved (asleep / static), else the smallest body id
 * of the island (island membership is compared as a set partition). */
int b2hip_get_island_labels(b2hip_world* w, int cap, int32_t* out);
/* Fat AABB of a fixture's proxy (b2BroadPhase::GetFatAABB). */
int b2hip_get_fat_aabb(b2hip_world* w, int fixture, float out4[4]);
/* The fat AABBs of fixtures [first, first + count) in one copy: what b2World::QueryAABB / RayCast walk
 * (b2World.cpp:1740-1795; the reference asks its dynamic tree, b2DynamicTree.h:168-287 - same boxes, other order). */
int b2hip_get_fat_aabbs(b2hip_world* w, int first, int count, float* out4n);

/* Test hook: FNV-1a hash of a group of device arrays (0 bodies, 1 contacts, 2 proxy AABBs, 3 contact impulses),
 * usable between phase calls to compare two worlds phase by phase. */
int b2hip_debug_hash(b2hip_world* w, int which, uint64_t* out);
/* With B2HIP_TRACE=1 in the environment at world creation, b2hip_solve records a (stage label, state hash)
 * per solver stage; returns 1 past the end. */
int b2hip_debug_trace(b2hip_world* w, int index, char* label, int label_cap, uint64_t* hash);
/* Raw read-back of one device array (see b2hip.hip for the ids); test / debugging only. */
int b2hip_debug_read(b2hip_world* w, int which, int first, int count, void* out);
/* Test hook: the world's stable LSD radix sort (the pair update's) over the caller's arrays: `count` keys with two payload
 * ints each are sorted in place by `passes` passes over the bits [shifts[p], shifts[p] + widths[p]), widths of 1 to 11. */
int b2hip_test_radix_sort(b2hip_world* w, int count, uint64_t* keys, int* payloads, int passes, const int* shifts, const int* widths);
/* Test hook: checks the contact-key set the pair update keeps across steps (B2HIP_KEYSET_KEEP) against the contact array.
 * Synchronises, reads only. out[0] 1 if the set is kept now (valid and not stale), [1] keys of live contacts the set does
 * not hold, [2] live entries minus live contacts (entries of dead contacts that survived), [3] recounted minus tracked
 * fill, [4] live entries, [5] tombstones. A kept set is right when [1] = [2] = [3] = 0. */
int b2hip_test_keyset_check(b2hip_world* w, long long out[6]);
/* Test hook: the world's storage. out[0] blocks of device and pinned host memory the library's owner types hold in this
 * process right now, all worlds together (w may be null): back at its earlier value once a world is destroyed. out[1] device
 * arrays of `w` whose pointer in the kernels' argument block is not the array's current one (0 for a null world): always 0. */
int b2hip_test_storage(b2hip_world* w, long long out[2]);

/* World snapshot (checkpoint / resume; the reference only has the lossy text b2World::Dump, b2World.cpp:2107-2164).
 * Everything that survives a step: bodies, shapes, fixtures with their proxy ids and fat AABBs, joints with their
 * accumulated impulses, the contact array in creation order with manifolds, warm-start impulses, cached impacts,
 * colours and TOI slots, the move buffer and the counters. A world loaded from it continues bit for bit like the world
 * it was taken from. The blob is only meaningful to the same build of the library.
 *   b2hip_save_snapshot: writes at most `cap` bytes; *needed receives the snapshot's size (call with cap 0 to ask).
 *   b2hip_load_snapshot: creates a NEW world (destroy it with b2hip_world_destroy); `device` as in b2hip_world_def. */
int b2hip_save_snapshot(b2hip_world* w, void* buffer, size_t cap, size_t* needed);
int b2hip_load_snapshot(const void* buffer, size_t size, int device, b2hip_world** out);

/* The state read-back of a step (40 B per body, the reference's b2Body members the user reads between steps, b2Body.h:126-131
 * GetTransform / GetPosition / GetAngle / velocities). Default (0): every step ends with it - b2hip_step returns with the rows on
 * the host. Lazy (1): a step ends with the counters only and the rows stay in HBM until the first call that needs a body's
 * state (b2hip_get_body_states, an edit of a body, a snapshot) fetches them, once; a caller that steps several times between
 * looks - or never looks, a batch run that reads the last state only - does not pay 40 MB of PCIe per step at 1 M bodies.
 * Results are the same bit for bit. B2HIP_LAZY_READBACK=1 in the environment sets it for every world created afterwards. */
int b2hip_set_lazy_readback(b2hip_world* w, int enable);

/* 13 floats in b2Profile declaration order (b2TimeStep.h:25-40), milliseconds, from HIP events. */
int b2hip_get_profile(b2hip_world* w, float ms[13]);
int b2hip_get_counters(b2hip_world* w, b2hip_counters* out);

/* Measurement hooks used by bench.py: mean duration (ms) of the solver kernel launches of the last
 * step measured with HIP events on the world's stream, and the algorithmic bytes they processed
 * (Ct*(Nv*220 + Np*136 + 488) + B*240). */
int b2hip_get_solver_timing(b2hip_world* w, float* ms, double* algorithmic_bytes, int* constraints, int* bodies);

/* Per-launch timing of the dominant solver kernel (k_large_velocity for coloured large islands, k_solve_small
 * for in-LDS small islands): when enabled, every launch of it is bracketed by a HIP event pair on the world's
 * stream. b2hip_get_kernel_timing reports, for the last step, the kernel's name, the SUM of its launch
 * durations (ms), the launch count and the algorithmic bytes those launches processed (220 B per constraint
 * per velocity sweep, resp. the whole 8d formula for the fused small-island kernel). Off by default: the event
 * pairs cost host time, so the timed region of bench.py runs without them. */
/* `enable`: 0 off, 1 the dominant solver kernel (above); 2 k_collide, 3 k_sync_fixtures, 4 k_find_pairs_small - the bandwidth
 * kernels of the other phases (one event pair per launch). Their algorithmic bytes are the SURVEY 8d per-unit figures times
 * the units the caller states with b2hip_set_kernel_timing_units (it knows the scene: collide = 480 B x contacts between two
 * polygons (units_a) + 230 B x other contacts (units_b); sync fixtures = 250 B x proxies (units_a); pair search = 16 B x proxies
 * (units_a) + 8 B x candidate pairs (units_b)). */
int b2hip_set_kernel_timing(b2hip_world* w, int enable);
int b2hip_set_kernel_timing_units(b2hip_world* w, long long units_a, long long units_b);
int b2hip_get_kernel_timing(b2hip_world* w, char* name, int name_cap, float* total_ms, int* launches, double* algorithmic_bytes);

/* ---- Batched world queries on the device (csrc/b2hip_api_query.h, csrc/b2d_kernels_query.h) ------------------------------
 * Many AABB, point or closest-ray queries in one blocking call, answered from the world's device state between steps:
 * every query sees the world that b2hip_get_fat_aabbs / b2hip_get_body_states report at the moment of the call (edits made
 * since the last step are uploaded first, as the next step would upload them; a world that is queried steps bit for bit
 * like one that is not). b2World::QueryAABB / RayCast keep their host path; these are for batches (sensor sweeps, lidar).
 *
 * filter: a fixture is a candidate when (category_bits & mask) != 0 and (include_sensors || !is_sensor). NULL means
 *   {0xFFFF, 1}: exactly the fixtures b2World::QueryAABB / RayCast consider.
 * fixture ids are device fixture ids (b2Fixture::GetDeviceId() + child index for a chain); body ids are device body ids.
 *
 * b2hip_query_aabbs: boxes = 4n floats (lower.x, lower.y, upper.x, upper.y). Reports every live proxy whose fat AABB
 *   overlaps the box, touching included (b2TestOverlap, the set b2World::QueryAABB reports), once, in ascending fixture
 *   id. A box with lower > upper or a NaN coordinate reports nothing.
 * b2hip_query_points: points = 2n floats. Reports the proxies whose fat AABB contains the point and whose shape contains it
 *   at the body's transform (b2Fixture::TestPoint; edges and chains contain no point), in ascending fixture id.
 * Both: offsets[n + 1] (offsets[i] .. offsets[i + 1] are query i's items, offsets[n] the total) are always complete;
 *   items receives the first min(total, cap) entries. Returns the total (>= 0) or a b2hip_status: when it exceeds cap,
 *   call again with cap = the total.
 * b2hip_ray_cast_closest: rays = 4n floats (p1.x, p1.y, p2.x, p2.y). out[i] is the hit that b2World::RayCast reports last
 *   to a callback returning the reported fraction: fraction and normal from the shape's ray cast, point = (1 - fraction)
 *   * p1 + fraction * p2. A miss, a zero-length ray or a NaN coordinate gives fixture = body = -1. Where two fixtures are
 *   hit at the same fraction the LOWEST fixture id is reported (the reference keeps the one its tree visits last).
 *   Returns B2HIP_OK or a b2hip_status.
 * Cost: a box, point or ray is answered from the cells of the broad-phase grid it can reach. A box window of more than
 *   4096 grid cells, a ray longer than 4096 cells, or a coordinate beyond 1e8 in magnitude tests every proxy of the world
 *   from one wave instead (10^6 candidates per query on a 10^6-body world). A box or point query with more than 4096 items
 *   is put in order by two extra launches, one after the other from the host, the second one workgroup reading a flag
 *   per proxy of the world.
 * All three: n <= 2^24 (more: B2HIP_ERR_INVALID); inside an open step B2HIP_ERR_INVALID; on a sharded world
 *   (b2hip_set_shard with more than one rank, b2hip_shard_spatial) B2HIP_ERR_UNSUPPORTED. Results are the same bytes run
 *   after run. The call runs on the world's stream and returns when the results are on the host. */
typedef struct b2hip_query_filter
{
	uint16_t mask;
	int include_sensors;
} b2hip_query_filter;
typedef struct b2hip_query_item
{
	int32_t fixture, body;
} b2hip_query_item;
typedef struct b2hip_ray_hit
{
	int32_t fixture, body;
	float point_x, point_y, normal_x, normal_y, fraction;
	int32_t pad;
} b2hip_ray_hit;
#define B2HIP_QUERY_MAX (1 << 24)
int b2hip_query_aabbs(b2hip_world* w, int n, const float* boxes4n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                      b2hip_query_item* items);
int b2hip_query_points(b2hip_world* w, int n, const float* points2n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                       b2hip_query_item* items);
int b2hip_ray_cast_closest(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, b2hip_ray_hit* out);

/* ---- Batched shape queries on the device (same file, same kernels) --------------------------------------------------------
 * The overlap and the closest linear cast of a convex shape, for many poses in one blocking call, on the same terms as the
 * block above: the world of b2hip_get_fat_aabbs / b2hip_get_body_states at the call, pending edits uploaded first, the
 * filter and the ids as above, refused inside an open step (B2HIP_ERR_INVALID) and on a sharded world
 * (B2HIP_ERR_UNSUPPORTED), the same bytes run after run, a queried world stepping bit for bit like one that is not.
 *
 * shapes: n_shapes b2hip_shape records as b2hip_create_fixture takes them - a circle, an edge, a polygon (1 to 8 vertices)
 *   or one child of a chain (type B2HIP_SHAPE_CHAIN, verts[0..3] the link's two vertices). A query names its shape by index,
 *   so one probe shape serves any number of poses. A pose (x, y, angle) becomes a transform on the host (sinf / cosf, as
 *   b2Rot::Set). A shape b2hip_create_fixture refuses, a polygon of no vertex, an index outside [0, n_shapes), n or
 *   n_shapes outside [0, 2^24], a NULL input or output: B2HIP_ERR_INVALID before any device work.
 * b2hip_query_shapes: every live proxy that passes the filter, whose fat AABB overlaps the query shape's AABB at the pose
 *   (b2Shape::ComputeAABB; touching included), and whose shape overlaps the query shape there: b2TestOverlap(query shape,
 *   0, fixture shape, child, pose, body transform), GJK distance with the radii below 10 FLT_EPSILON. Once each, in
 *   ascending fixture id; offsets / cap / the returned total exactly as b2hip_query_aabbs. A NaN in a pose reports nothing.
 * b2hip_shape_cast_closest: the query shape moves from its pose by (tx, ty). Candidates are the live proxies that pass the
 *   filter and whose fat AABB overlaps the sweep box (the union of the shape's AABB at the pose and at the pose moved by
 *   the translation); a candidate is hit when b2ShapeCast returns true with proxyA = the fixture's child at its body's
 *   transform, proxyB = the query shape at the pose, translationB = (tx, ty) (the operand order of the Testbed's
 *   ShapeCast test). out[i] is the hit of the smallest (lambda, fixture id): fraction = lambda, point and normal from
 *   b2ShapeCast. A miss, a NaN or a non-finite translation gives fixture = body = -1, fraction = 1.
 *   Start in overlap: a fixture whose core the shape's core already overlaps at its pose is NOT a hit (b2ShapeCast returns
 *   false for it), and one whose skin alone it overlaps is hit at lambda 0 (b2ShapeCast's answer as well): ask
 *   b2hip_query_shapes for what the shape overlaps at the start pose.
 * Cost: each query or cast is one wave over the broad-phase grid. A query box or sweep box whose window has more than 4096
 *   grid cells is walked in cell-long pieces of the translation (casts) or tests every proxy of the world (overlaps, and
 *   casts longer than 4096 cells); so does a coordinate beyond 1e8 in magnitude. An overlap query with more than 4096 items
 *   is put in order by two extra launches, as in b2hip_query_aabbs. Every candidate costs a GJK distance or shape cast. */
typedef struct b2hip_shape_query
{
	int32_t shape;
	float x, y, angle;
} b2hip_shape_query; /* 16 bytes */
typedef struct b2hip_shape_cast
{
	int32_t shape;
	float x, y, angle, tx, ty;
	int32_t pad[2];
} b2hip_shape_cast; /* 32 bytes */
int b2hip_query_shapes(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_query* queries,
                       const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_query_item* items);
int b2hip_shape_cast_closest(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_cast* casts,
                             const b2hip_query_filter* f, b2hip_ray_hit* out);

/* ---- Batched distance queries on the device (same file, same kernels) -----------------------------------------------------
 * How far the nearest fixture is and where (b2hip_shape_distance_closest), or every fixture within a range with its
 * distance and closest points (b2hip_query_shapes_within), for many poses of a convex shape in one blocking call; on the
 * same terms as the two blocks above: the world of b2hip_get_fat_aabbs / b2hip_get_body_states at the call, pending edits
 * uploaded first, the filter, the ids and the shape table as above, refused inside an open step (B2HIP_ERR_INVALID) and on
 * a sharded world (B2HIP_ERR_UNSUPPORTED), the same bytes run after run, a queried world stepping bit for bit like one
 * that is not. Each call runs on the world's stream and returns when the results are on the host.
 *
 * Candidates: the query box is the query shape's AABB at the pose (b2Shape::ComputeAABB) with max_distance subtracted from
 *   both lower coordinates and added to both upper ones (one float operation each). The candidates are exactly the live
 *   proxies that pass the filter and whose fat AABB overlaps that box, touching included: the set b2World::QueryAABB
 *   reports over it. So the answer does not depend on how the grid is walked. (A fat AABB holds its fixture's shape, so a
 *   fixture within max_distance is a candidate; only a chain link's box leaves its b2_polygonRadius skin out.)
 * Value: b2Distance with proxyA = the query shape (child 0) at the pose, proxyB = the fixture's child at its body's
 *   transform, useRadii = true and a zeroed cache - the orientation of b2TestOverlap and b2hip_query_shapes. point_a lies
 *   on the query shape, point_b on the fixture, both on the skins (the radii are applied); iterations is
 *   b2DistanceOutput::iterations. A candidate counts when distance <= max_distance. Shapes that overlap give distance 0
 *   and both points at the midpoint of the cores' closest points, as b2Distance does. max_distance = 0 therefore reports
 *   the fixtures at distance == 0 only: NOT the `< 10 FLT_EPSILON` rule of b2hip_query_shapes, which also passes a
 *   positive distance below that bound.
 * b2hip_shape_distance_closest: out[i] is the candidate with the smallest (distance, fixture id): distances are >= +0, so
 *   their bits order like their values, and ties go to the LOWER fixture id. Nothing within range: fixture = body = -1,
 *   the four point coordinates 0, iterations = 0, distance = +infinity. Returns B2HIP_OK or a b2hip_status.
 * b2hip_query_shapes_within: every counting candidate once, in ascending fixture id, each with its full record. offsets
 *   (n + 1) are always complete, hits receives the first min(total, cap) records, the total is returned (or a
 *   b2hip_status): when it exceeds cap, call again with cap = the total - exactly as b2hip_query_aabbs.
 * Invalid records: a pose with a NaN or non-finite component, a max_distance that is NaN, negative or infinite. The closest
 *   call answers one with the miss above, the within call with an empty list.
 * Argument errors, refused with B2HIP_ERR_INVALID before any device work: n or n_shapes outside [0, 2^24], a NULL input or
 *   output, a negative cap, a shape b2hip_create_fixture refuses, a polygon of no vertex, a shape index outside
 *   [0, n_shapes).
 * Cost: one wave per query. The closest call visits the large proxies, then the grid cells around the shape's box in
 *   rings of 1, 2, 4, ... cells and stops once the best distance found is below the ring's reach: something near costs a
 *   few cells whatever max_distance is. With nothing near it walks out to the whole query box, and a ring of more than
 *   4096 grid cells - or a coordinate beyond 1e8 in magnitude - tests every proxy of the world from that one wave (10^6
 *   candidates on a 10^6-body world): the slow case, so keep max_distance near what the caller needs. The within call
 *   walks the whole query box in a count and a fill pass (more than 4096 cells: every proxy, twice), sorts, and evaluates
 *   each reported record once more; a list of more than 4096 records is put in order by two extra launches, as in
 *   b2hip_query_aabbs. Every candidate costs a GJK distance. */
typedef struct b2hip_shape_range
{
	int32_t shape;       /* index into `shapes` */
	float x, y, angle;   /* pose of the query shape */
	float max_distance;  /* finite, >= 0 */
	int32_t pad;
} b2hip_shape_range; /* 24 bytes */
typedef struct b2hip_distance_hit
{
	int32_t fixture, body;   /* -1, -1: nothing within range */
	float point_ax, point_ay; /* closest point on the query shape */
	float point_bx, point_by; /* closest point on the fixture */
	float distance;
	int32_t iterations;      /* b2DistanceOutput::iterations */
} b2hip_distance_hit; /* 32 bytes */
int b2hip_shape_distance_closest(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_range* ranges,
                                 const b2hip_query_filter* f, b2hip_distance_hit* out);
int b2hip_query_shapes_within(b2hip_world* w, int n_shapes, const b2hip_shape* shapes, int n, const b2hip_shape_range* ranges,
                              const b2hip_query_filter* f, int cap, int32_t* offsets, b2hip_distance_hit* hits);

/* ---- Batched all-hit and any-hit ray casts on the device (same file, same kernels) ----------------------------------------
 * Every fixture a ray crosses (b2hip_ray_cast_all: multi-return lidar, projectiles that penetrate, what lies between A and
 * B) or whether it crosses one at all (b2hip_ray_cast_any: line of sight, one byte per ray), for many rays in one blocking
 * call; on the same terms as the blocks above: the world of b2hip_get_fat_aabbs / b2hip_get_body_states at the call,
 * pending edits uploaded first, the filter and the ids as above, the same bytes run after run, a queried world stepping bit
 * for bit like one that is not. Each call runs on the world's stream and returns when the results are on the host.
 *
 * rays: 4n floats (p1.x, p1.y, p2.x, p2.y), as b2hip_ray_cast_closest takes them.
 * Hit set of ray i: every live proxy that passes the filter and whose shape's ray cast (b2Shape::RayCast at the body's
 *   transform with p1, p2 and maxFraction = 1) returns true: the set b2World::RayCast reports to a callback that returns 1
 *   for the fixtures the filter passes and -1 for the others. Each proxy appears once; a chain's child is a fixture id of
 *   its own. A ray that starts inside a polygon does not hit it (b2PolygonShape::RayCast).
 * Record: a b2hip_ray_hit exactly as b2hip_ray_cast_closest fills it - fraction and normal from the shape's ray cast, point
 *   = (1 - fraction) * p1 + fraction * p2, pad = 0.
 * Order: ascending by (bits of fraction + 0.0f, fixture id): a fraction of -0.0 (a ray that starts on an edge or a circle)
 *   sorts as +0.0 and is reported as it is, and ties go to the LOWER fixture id. So hits[offsets[i]] is bit for bit what
 *   b2hip_ray_cast_closest returns for ray i.
 * b2hip_ray_cast_all: offsets (n + 1) are always complete, hits receives the first min(total, cap) records, the total is
 *   returned (or a b2hip_status): when it exceeds cap, call again with cap = the total - exactly as b2hip_query_aabbs. A
 *   total above 2^31, or more than 2^30 hits of one ray: B2HIP_ERR_CAPACITY.
 * b2hip_ray_cast_any: out[i] = 1 when the hit set of ray i is not empty, else 0; for every input this is
 *   b2hip_ray_cast_closest(...)[i].fixture >= 0. Returns B2HIP_OK or a b2hip_status.
 * Invalid rays: a zero-length ray or a coordinate that is not finite gives an empty list / 0.
 * Argument errors, refused with B2HIP_ERR_INVALID before any device work and before the world is looked at: n outside
 *   [0, 2^24], a NULL input or output, a negative cap. Then: a NULL world, or a call inside an open step,
 *   B2HIP_ERR_INVALID; a sharded world (b2hip_set_shard with more than one rank, b2hip_shard_spatial)
 *   B2HIP_ERR_UNSUPPORTED.
 * Cost: one wave per ray over the broad-phase grid, in pieces a cell long. A ray of more than 4096 pieces, or a coordinate
 *   beyond 1e8 in magnitude, tests every proxy of the world from its one wave instead (10^6 candidates on a 10^6-body
 *   world) - twice in the all-hit call, which counts and then fills. The all-hit call walks the WHOLE ray where the closest
 *   call stops at the first piece that holds a hit, casts every reported fixture once more for its record, and sorts each
 *   ray's list in LDS; a ray with more than 4096 hits is sorted in global memory by one workgroup, one launch per such ray,
 *   one after the other from the host: correct, and slow. The any-hit call stops at the first piece that holds a hit and
 *   copies one byte per ray back. */
int b2hip_ray_cast_all(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, int cap, int32_t* offsets,
                       b2hip_ray_hit* hits);
int b2hip_ray_cast_any(b2hip_world* w, int n, const float* rays4n, const b2hip_query_filter* f, uint8_t* out);

/* ---- Batched per-body contact lists and contact totals on the device (csrc/b2hip_api_body_contacts.h,
 * csrc/b2d_kernels_body_contacts.h) -------------------------------------------------------------------------------------------
 * What touches each of my bodies, and how hard: the touch sensor, the foot contact, the force sensor of many agents, in one
 * blocking call between steps, without copying the world's contacts (96 bytes each) to the host. Both calls only read: a
 * world on which they are used steps bit for bit like one on which they are not, and the same call gives the same bytes run
 * after run.
 *
 * bodies: n body ids, each in [0, b2hip_body_count) and each at most once.
 * The list of body b: every contact k of b2hip_get_contacts, as that call would answer at the same moment, with
 *   body_a == b || body_b == b; with touching_only != 0 only those with flags & 1. Each appears once, in ascending
 *   contact_index. A contact between two bodies of the batch appears in both lists. A destroyed body has an empty list.
 * Edits made since the last step are seen as b2hip_get_contacts / b2hip_get_body_states see them: the host mirror is uploaded
 *   and the queued contact-array operations are applied first, so the contacts of a body destroyed since the step are gone,
 *   contact_index agrees with b2hip_get_contacts called next, and a transform set since the step is the one the normals use.
 * Record (b2hip_body_contact): fixture is this body's fixture id and other_fixture the other body's (a chain's child is a
 *   fixture id of its own, as in b2hip_contact).
 *   normal: b2WorldManifold::Initialize's normal for the contact's manifold and the two bodies' current transforms (the
 *   points are not computed, so no radii enter), with the sign + when this body is body_b and - when it is body_a: it
 *   points from the other body towards this one. b2ContactSolver applies P = jn n + jt cross(n, 1) as -P to A and +P to B,
 *   so with this orientation the impulse on THIS body is normal_impulse * normal + tangent_impulse * (normal.y, -normal.x)
 *   on either side.
 *   normal_impulse / tangent_impulse: the sum over the manifold points j < point_count - a one-point contact's is that
 *   point's, a two-point contact's is imp0 + imp1 (one fp32 add). A contact with point_count == 0 (a sensor overlap, a
 *   contact that is not touching) has normal = (0, 0) and zero impulses.
 * b2hip_body_contacts: offsets (n + 1) are always complete, records receives the first min(total, cap) records, the total
 *   is returned (or a b2hip_status): when it exceeds cap, call again with cap = the total - exactly as b2hip_query_aabbs.
 * b2hip_body_contact_totals: one record per body over its TOUCHING records: contacts counts every entry of
 *   b2hip_get_contacts that names the body, touching those of them that touch; impulse is the sum of the touching records'
 *   impulse vectors (above), normal_impulse the sum and max_normal_impulse the largest of their normal_impulse (0 without a
 *   touching contact), points the sum of their point_count, pad 0. The sums are fp32, formed in an order that depends only on
 *   the body's list (no float atomics anywhere); the order is otherwise not part of the contract. Returns B2HIP_OK or a
 *   b2hip_status. A destroyed body, or one without contacts, has an all-zero total.
 * Argument errors, refused with B2HIP_ERR_INVALID before any device work and before the world is looked at, in this order:
 *   n outside [0, 2^24]; a negative cap; a NULL offsets / out, NULL bodies with n > 0, NULL records with cap > 0. Then the
 *   world: a NULL world, or a call inside an open step, B2HIP_ERR_INVALID; a sharded world (b2hip_set_shard with more than one
 *   rank, b2hip_shard_spatial) B2HIP_ERR_UNSUPPORTED. Then the ids, on the host, before any device work: an id outside
 *   [0, b2hip_body_count) or one that occurs twice is B2HIP_ERR_INVALID, and b2hip_last_error names the first offender.
 *   n == 0 writes offsets[0] = 0 and returns 0.
 * Cost: two passes over the world's contact array (20 bytes a contact each: ids and flags), a scan over the batch, a sort of
 *   each body's list in LDS, then one thread per record (lists) or one wave per body (totals). A body with more than 4096
 *   listed contacts (a container, a ground under a crowd) is ordered by marking its contacts in a flag per contact of the
 *   world and compacting the flags from ONE workgroup, one such body after the other from the host: correct, and slow. */
typedef struct b2hip_body_contact       /* 32 bytes */
{
	int32_t contact_index;          /* index into b2hip_get_contacts called at the same point */
	int32_t other_body;
	int32_t fixture, other_fixture; /* this body's fixture id, the other body's (a chain child is its own id) */
	float normal[2];                /* world manifold normal, pointing from the other body towards this one */
	float normal_impulse;           /* sum over the manifold points j < point_count */
	float tangent_impulse;          /* likewise */
} b2hip_body_contact;

typedef struct b2hip_body_contact_total /* 32 bytes */
{
	int32_t contacts;               /* entries of b2hip_get_contacts that name the body */
	int32_t touching;               /* of those, touching (flags bit0) */
	float impulse[2];               /* net impulse the touching contacts put on this body in the last step, world frame */
	float normal_impulse;           /* sum of the touching records' normal_impulse */
	float max_normal_impulse;       /* largest of them; 0 with no touching contact */
	int32_t points;                 /* manifold points of the touching contacts */
	int32_t pad;                    /* 0 */
} b2hip_body_contact_total;

int b2hip_body_contacts(b2hip_world* w, int n, const int32_t* bodies, int touching_only, int cap, int32_t* offsets /* n + 1 */,
                        b2hip_body_contact* records /* cap */);
int b2hip_body_contact_totals(b2hip_world* w, int n, const int32_t* bodies, b2hip_body_contact_total* out /* n */);

/* ---- F. Batched body writes on the device (csrc/b2hip_api_body_writes.h, csrc/b2d_kernels_body_writes.h) ---------------------
 * Push many bodies between two steps in one call: the control loop of many agents, a crowd, wind, an explosion. The
 * single-body calls (b2hip_apply_force, b2hip_set_velocity, b2hip_apply_*_impulse) edit the host's mirror, and the next step
 * uploads eight rows per edited body; these calls edit the device's rows in one launch and the host's mirror follows.
 *
 * Definition by equivalence. Each write call has the effect of the existing single-body calls made for i = 0 .. n-1 in
 * order, to the bit, for everything a caller can observe afterwards: b2hip_get_body_states, later single-body edits,
 * snapshots, every later step. With s the state b2hip_get_body_states reports for bodies[i] at the call:
 *   b2hip_apply_forces:   b2hip_apply_force(w, b, x, y, T, wake) with T = angular when at_point == 0, else
 *                         T = angular + ((px - s.cx) * y - (py - s.cy) * x) in float32, in that operation order.
 *   b2hip_apply_impulses: first the linear call - b2hip_apply_linear_impulse_to_center(w, b, x, y, wake) when at_point == 0,
 *                         b2hip_apply_linear_impulse(w, b, x, y, px, py, wake) otherwise - then
 *                         b2hip_apply_angular_impulse(w, b, angular, wake). Both are always made: a zero still does its +=.
 *   b2hip_set_velocities: b2hip_set_velocity(w, b, vx', vy', w') with the primed values from v3 where the mask bit is set
 *                         (bit 0: the linear velocity, bit 1: the angular velocity) and from s where it is not; the wake rule
 *                         of b2hip_set_velocity (a non-zero velocity wakes the body and restarts its sleep timer) is applied
 *                         to the primed values.
 *   So: forces and impulses skip bodies that are not dynamic, velocities skip static bodies; a sleeping body with wake == 0 is
 *   left alone; waking sets the awake flag and zeroes the sleep time.
 * Order: edits made before the call lie underneath it and edits made after it on top of it, as in the loop: a single
 *   b2hip_apply_force after b2hip_apply_forces adds to the batch's sum, a b2hip_set_velocity replaces the batch's velocity.
 *   Two write calls before one step act one after the other.
 * bodies: n body ids, each in [0, b2hip_body_count), not destroyed, and each AT MOST ONCE per write call - that is what makes
 *   a call deterministic without atomics. (To push a body twice, make two calls.)
 * b2hip_get_body_states_of: the b2hip_body_state rows of n bodies - out[i] is what b2hip_get_body_states reports for
 *   bodies[i] at the same moment - gathered on the device: n x 40 bytes cross, not the table, whatever
 *   b2hip_set_lazy_readback says and without fetching the table. A read: an id may occur more than once.
 * Argument errors, refused with B2HIP_ERR_INVALID before the world is looked at, in this order: n outside [0, 2^24]; a NULL
 *   bodies / push / v3 with n > 0, a NULL out; a mask other than 1, 2 or 3. Then the world: a NULL world, or a call inside an
 *   open step (a listener's callback window included), B2HIP_ERR_INVALID; a sharded world (b2hip_set_shard with more than one
 *   rank, b2hip_shard_spatial) B2HIP_ERR_UNSUPPORTED. Then the ids, on the host, before any device work: an id out of range, a
 *   destroyed body or (write calls) an id that occurs twice is B2HIP_ERR_INVALID, and b2hip_last_error names the first
 *   offender by entry and id. A refused call applies nothing. n == 0 is a successful no-op. All four return B2HIP_OK or a
 *   b2hip_status.
 * Cost: the ids and records cross in one copy, one launch edits one body per lane, and the call returns when the device is
 *   done; nothing comes back. The body-state table is not fetched: the rows are marked as newer on the device, and the next
 *   b2hip_get_body_states (or single-body edit) fetches the rows that changed. */
typedef struct b2hip_body_push {        /* 32 bytes */
	float   x, y;        /* force [N] or linear impulse [N s], world frame */
	float   angular;     /* torque [N m] or angular impulse */
	int32_t at_point;    /* 0: at the centre of mass; 1: at the world point (px, py) */
	float   px, py;
	int32_t pad[2];
} b2hip_body_push;

int b2hip_apply_forces  (b2hip_world* w, int n, const int32_t* bodies, const b2hip_body_push* push, int wake);
int b2hip_apply_impulses(b2hip_world* w, int n, const int32_t* bodies, const b2hip_body_push* push, int wake);
/* v3: n x (vx, vy, omega); mask bit 0: set the linear velocity, bit 1: set the angular velocity (1, 2 or 3) */
int b2hip_set_velocities(b2hip_world* w, int n, const int32_t* bodies, const float* v3, int mask);
/* the b2hip_body_state rows of n bodies, gathered on the device: n x 40 bytes cross, not the table */
int b2hip_get_body_states_of(b2hip_world* w, int n, const int32_t* bodies, b2hip_body_state* out);

/* ---- G. Batched joints on the device (csrc/b2hip_api_joint_batch.h, csrc/b2d_kernels_joint_batch.h) -------------------------
 * Drive and read many joints between two steps in one call each: the motor targets of arms, cars, ragdolls and walkers, and
 * what their joints did. b2hip_joint_set_motor queues one upload per joint and puts both bodies through the host's mirror
 * (eight rows uploaded per body); b2hip_get_joint_reaction and b2hip_get_joint_limit_state copy and wait once per joint. These
 * calls do either in one launch.
 *
 * b2hip_joint_set_motors. mask bit 1: enable_motor, bit 2: motor_speed, bit 4: max_motor (max_motor is the maximum motor
 *   torque of a revolute or wheel joint, the maximum motor force of a prismatic joint).
 *   Definition by equivalence: the call has the effect of b2hip_joint_set_motor(w, joints[i], e', s', m') made for
 *   i = 0 .. n-1 in order, with a primed value from motors[i] where its mask bit is set and otherwise the value the joint
 *   currently has (what a preceding b2hip_joint_set_motor or batch left) - to the bit, for everything a caller can observe
 *   afterwards: b2hip_get_body_states, b2hip_get_joint_states, later single edits, snapshots, every later step.
 *   So: an entry whose primed triple equals the current one does nothing and wakes nobody. An entry that changes its joint
 *   does b2Body::SetAwake(true) on both of its bodies: the awake flag is set and the sleep time zeroed whether or not the
 *   body slept; a static body that is awake already is left untouched. Joints of one batch may share bodies (a chain, a
 *   chassis with two wheels): every writer stores the same values, so the result does not depend on the order of the lanes.
 *   joints: n joint ids, each in [0, b2hip_joint_count), not destroyed, revolute, prismatic or wheel, and each AT MOST ONCE per
 *   call. (To set a joint twice, make two calls.)
 *   Order: edits made before the call lie underneath it and edits made after it on top of it, as in the loop: a
 *   b2hip_joint_set_motor before a batch whose mask omits the speed keeps its speed, a b2hip_joint_set_limits after a batch
 *   keeps the batch's motor. Two calls before one step act one after the other.
 * b2hip_get_joint_states. A read: an id may occur more than once and the world is not changed. Per entry:
 *   type         the joint's type (0 revolute, 1 distance, 2 prismatic, 3 weld, 4 wheel, 5 rope, 6 friction, 7 motor,
 *                8 pulley, 9 mouse, 10 gear). A destroyed joint gives -1 and zeros in every other member.
 *   limit_state  what b2hip_get_joint_limit_state returns at that moment.
 *   force, torque, motor   what b2hip_get_joint_reaction(w, joint, inv_dt, ..) returns, to the bit. inv_dt is taken as given.
 *   coordinate, speed, coordinate2, speed2   the getters of the joint classes, in float32, from the bodies' current states:
 *                revolute   GetJointAngle (aB - aA - reference angle), GetJointSpeed (wB - wA), 0, 0
 *                prismatic  GetJointTranslation, GetJointSpeed, 0, 0
 *                wheel      GetJointTranslation, GetJointLinearSpeed, GetJointAngle (aB - aA), GetJointAngularSpeed
 *                pulley     GetCurrentLengthA, 0, GetCurrentLengthB, 0
 *                every other type: zeros
 *   Body edits made since the step (b2hip_set_transform, a batched velocity set) are seen: the pending edits are uploaded
 *   before the launch. A joint created since the last step reports a zero reaction and its coordinates from the bodies.
 * Argument errors, refused with B2HIP_ERR_INVALID before the world is looked at, in this order: n outside [0, 2^24]; a NULL
 *   joints / motors with n > 0, a NULL out; a mask outside 1..7. Then the world: a NULL world, or a call inside an open step (a
 *   listener's callback window included), B2HIP_ERR_INVALID; a sharded world (b2hip_set_shard with more than one rank,
 *   b2hip_shard_spatial) B2HIP_ERR_UNSUPPORTED. Then the ids, on the host, before any device work: an id outside
 *   [0, b2hip_joint_count), and for b2hip_joint_set_motors a destroyed joint, a joint whose type has no motor or an id that
 *   occurs twice, is B2HIP_ERR_INVALID, and b2hip_last_error names the first offender by entry and id. A refused call
 *   applies nothing. n == 0 is a successful no-op. Both return B2HIP_OK or a b2hip_status.
 * Cost: b2hip_joint_set_motors sends the entries that change (16 bytes each) in one copy, one launch edits one joint per lane,
 *   and the call returns when the device is done; nothing comes back, and the body-state table is not fetched (the woken
 *   bodies' rows are marked as newer on the device). b2hip_get_joint_states sends 4 bytes and fetches 48 bytes per entry.
 * b2hip_joint_count: joints ever created (ids are never reused); b2hip_joint_is_destroyed: 1 for a destroyed joint, else 0. */
typedef struct b2hip_joint_motor {      /* 16 bytes */
	int32_t enable_motor;
	float   motor_speed;
	float   max_motor;   /* maximum motor torque (revolute, wheel) or force (prismatic) */
	int32_t pad;
} b2hip_joint_motor;

typedef struct b2hip_joint_state {      /* 48 bytes */
	int32_t type;        /* -1: destroyed */
	int32_t limit_state; /* b2hip_get_joint_limit_state */
	float   coordinate, speed;
	float   coordinate2, speed2;
	float   force[2];    /* b2hip_get_joint_reaction: on bodyB at the anchor */
	float   torque;
	float   motor;
	float   pad[2];      /* 0 */
} b2hip_joint_state;

int b2hip_joint_count(const b2hip_world* w);
int b2hip_joint_is_destroyed(const b2hip_world* w, int joint);
int b2hip_joint_set_motors(b2hip_world* w, int n, const int32_t* joints, const b2hip_joint_motor* motors, int mask);
int b2hip_get_joint_states(b2hip_world* w, int n, const int32_t* joints, float inv_dt, b2hip_joint_state* out);

/* ---- H. Batched teleports and sleep / wake sets on the device (csrc/b2hip_api_body_writes.h, csrc/b2d_kernels_body_writes.h) --
 * Move many bodies between two steps in one call, and put them to sleep or wake them: resetting agents or episodes to their
 * start poses, moving scripted platforms, respawning debris. b2hip_set_transform edits the host's mirror, waits for the
 * device and reads 16 bytes back per fixture, and the next step uploads eight rows per body and six small blocking copies
 * per moved proxy; these calls edit the device's rows, fat AABBs and move buffer in one launch. They are two more write
 * calls of block F's family and follow its conventions unless stated otherwise.
 *
 * Definition by equivalence. Each call has the effect of the existing single-body calls made for i = 0 .. n-1 in order, to
 * the bit, for everything a caller can observe afterwards: b2hip_get_body_states and b2hip_get_body_states_of,
 * b2hip_get_fat_aabb(s), batched queries made before the next step, later single-body edits, a snapshot that is loaded and
 * stepped, every later step's body states and contacts. (The order of the entries in the move buffer is not observable and
 * may differ: the pairs are sorted.) With s the state b2hip_get_body_states reports for bodies[i] at the call:
 *   b2hip_set_transforms: b2hip_set_transform(w, b, x', y', a') with x', y' from pose3 when mask bit 0 (value 1) is set, else
 *                         s.px, s.py, and a' from pose3 when mask bit 1 (value 2) is set, else s.angle.
 *     Per body: the transform becomes (x', y', sin a', cos a'), the centre c = xf * localCenter, the position row (c, a') with
 *     the sleep time unchanged, and the sweep origin (c, a'). Nothing else of the body changes: it does not wake, it keeps its
 *     velocity, and static and kinematic bodies move as well (b2Body.cpp:451-473).
 *     Per proxy of the body, newest first: the shape's AABB at the new transform; if the fat AABB contains it nothing
 *     happens; otherwise the fat AABB becomes that box grown by the AABB extension (0.1 m) on each side, with no displacement
 *     term, and the proxy is appended once to the move buffer. An inactive body has no proxies: its pose is set and no proxy
 *     row is touched.
 *   b2hip_set_awakes:     b2hip_set_awake(w, b, awake[i] != 0). False clears the awake flag and zeroes the sleep time, the
 *     velocity and the force and torque, on any body type. True sets the flag and zeroes the sleep time, except that a static
 *     body that is awake already is left untouched.
 * Order: edits made before the call lie underneath it - a body or fixture created since the last step can be named - and edits
 *   made after it on top of it: a b2hip_set_transform after a batch moves the body again, a b2hip_apply_force after
 *   b2hip_set_awakes(false) adds to zero. Two calls before one step act one after the other.
 * bodies: n body ids, each in [0, b2hip_body_count), not destroyed, and each AT MOST ONCE per call.
 * Refusals, in this order: n outside [0, 2^24], a NULL bodies / pose3 / awake with n > 0, a mask other than 1, 2 or 3:
 *   B2HIP_ERR_INVALID before the world is looked at. A NULL world, or a call inside an open step (a listener's callback window
 *   included): B2HIP_ERR_INVALID. A sharded world: B2HIP_ERR_UNSUPPORTED. An id out of range, a destroyed body or an id that
 *   occurs twice: B2HIP_ERR_INVALID, and b2hip_last_error names the first offender by entry and id. A refused call applies
 *   nothing. n == 0 is a successful no-op.
 * The move buffer. It holds 2 x fixtures + 64 entries and is emptied by the step. Neither the reference nor the single call
 *   removes duplicates from buffered moves, so repeated teleports of the same bodies between two steps can fill it.
 *   b2hip_set_transforms adds the live proxies of the named bodies - the most the call can append - to the moves the device
 *   has buffered, and if the sum does not fit it returns B2HIP_ERR_UNSUPPORTED, says to step first, and applies nothing. One
 *   batch over every body of a freshly stepped world always fits.
 * Cost: 4 + 12 bytes (transforms) or 4 + 1 bytes (awakes) per entry cross in one copy; one launch edits one body per lane, and
 *   the call returns when the device is done. b2hip_set_transforms reads the move counter (4 bytes) first; otherwise nothing
 *   comes back, and the body-state table is not fetched. A lane walks the proxy list of its body: a body with a long list (a
 *   container, a chain of edges) is walked by one lane, serially. */
/* pose3: n x (x, y, angle); mask: 1 position, 2 angle, 3 both */
int b2hip_set_transforms(b2hip_world* w, int n, const int32_t* bodies, const float* pose3, int mask);
/* awake: one byte per entry, 0 = SetAwake(false), non-zero = SetAwake(true) */
int b2hip_set_awakes(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* awake);

/* ---- I. Batched destruction and activation sets on the device (csrc/b2hip_api_body_lifecycle.h, csrc/b2d_kernels_body_lifecycle.h)
 * Retire many bodies for good, or switch them off and on again, between two steps in one call: debris that has left the
 * scene, projectiles that have hit, a pool of bodies that respawn. Body ids are never reused - a destroyed body is a dead slot
 * for the life of the world - so pooling with b2hip_set_actives is the way to respawn, and b2hip_destroy_bodies the way to
 * retire. The single calls queue one contact-array operation per body, each of which is a walk of ONE workgroup over the whole
 * contact array, and five small blocking copies per fixture; these calls edit the rows and the proxies in one launch each and
 * destroy the contacts of the whole set in one grid-wide pass. They are two more write calls of block F's family and follow
 * the conventions of b2hip_set_transforms unless stated otherwise.
 *
 * Definition by equivalence. A call has the effect of b2hip_destroy_body(w, bodies[i]), respectively
 * b2hip_set_active(w, bodies[i], active[i] != 0), made for i = 0 .. n-1 in order with nothing in between, to the bit, for
 * everything a caller can observe afterwards: b2hip_get_body_states / _of (the rows of dead bodies included),
 * b2hip_body_is_destroyed / b2hip_fixture_is_destroyed and the counts, b2hip_get_fat_aabb(s) of live proxies,
 * b2hip_get_contacts before and after later steps (contacts appear in proxy-id order), the contact events of the next step,
 * batched queries made before the next step, later single-body edits, a snapshot that is saved (and, where the world holds
 * no inactive body, loaded and stepped), every later step. (The order of the entries in the move buffer and of the events
 * appended within one call is not observable.) An entry of b2hip_set_actives that has the requested state already is a
 * no-op, as the single call is. b2hip_set_actives touches no joint, as the single call does not.
 * When the contacts go. The single calls queue the destruction of the contacts for the next step or the next reader of the
 *   contacts (b2hip_get_contacts, b2hip_contact_count, a batched call): until then b2hip_get_body_states does not show the
 *   bodies that the destroyed touching contacts wake. A batch destroys them before it returns (the loop it runs for a jointed
 *   body included: what the loop queued is applied before the call returns). Compare the two routes behind a read of the
 *   contacts. The end events of the destroyed contacts are delivered with the next step's events on either route.
 * Order: edits made before the call lie underneath it: they go to the device first, queued contact operations included - a
 *   body created since the last step can be named - and edits made after it on top of it. Two calls before one step act one
 *   after the other. This LIMITS the definition by equivalence to the call itself: single calls made before a batch, or two
 *   batches, are not the same as all their single calls queued together. Queued together, every body's rows are uploaded before
 *   any contact goes, so a body that an earlier call's destroyed contacts wake and a later call destroys or puts to sleep can
 *   end with another awake bit. A caller who mixes the routes gets the batch's order - each call complete before the next -
 *   which is what the single route gives with a read of the contacts (b2hip_contact_count) between the calls. The end events
 *   of single calls that a batch applies this way are delivered with the next step's, like the batch's own.
 * Joints. b2hip_destroy_body destroys the live joints of its body first, and b2hip_destroy_joint wakes both bodies in an order
 *   against the other entries' edits that can be observed. If any named body carries a live joint (a gear joint's third and
 *   fourth body count), b2hip_destroy_bodies runs the loop of b2hip_destroy_body itself for the whole batch - pending edits
 *   to the device first, and what the loop queued applied before the call returns, as on the batched route: the result is
 *   the same, the cost is the loop's.
 * bodies: n body ids, each in [0, b2hip_body_count), not destroyed, and each AT MOST ONCE per call.
 * Refusals, in this order: n outside [0, 2^24], a NULL bodies / active with n > 0: B2HIP_ERR_INVALID before the world is looked
 *   at. A NULL, failed or mid-step world (a listener's callback window included): B2HIP_ERR_INVALID. A sharded world:
 *   B2HIP_ERR_UNSUPPORTED. An id out of range, a destroyed body or an id that occurs twice: B2HIP_ERR_INVALID, and
 *   b2hip_last_error names the first offender by entry and id. A refused call applies nothing. n == 0 is a successful no-op.
 *   A B2HIP_ERR_HIP from these calls is no refusal: a copy, a launch or a sort failed behind the host's bookkeeping, the device
 *   is partly edited, and the world is marked failed - every later call says so, and it can only be inspected and destroyed.
 * Two refusals more, of b2hip_set_actives, both checked before anything is written:
 *   The move buffer. An activated proxy buffers a move. The call adds the proxies it would create to the moves the device has
 *     buffered, and if the sum does not fit (2 x fixtures + 64 entries, emptied by the step) it returns B2HIP_ERR_UNSUPPORTED,
 *     says to step first, and applies nothing.
 *   Proxy-id reuse. The ids the reference's tree would hand out are replayed in entry order on a copy of the allocator first.
 *     Where an internal node's id would become a leaf's (the broad-phase tree was emptied and refilled: not modelled) the call
 *     returns B2HIP_ERR_UNSUPPORTED, names the entry, and leaves the world untouched. This is the ONE place where a refused
 *     batch differs from a refused loop: b2hip_set_active returns the same code from the middle of its loop, with the earlier
 *     fixtures of that body - and the earlier bodies of the loop - already edited.
 * Cost: 4 + 4 bytes per entry and 16 bytes per fixture of a named body cross in one copy; the device's counters (about 2 KB)
 *   come back first. One pass over the contact array destroys the contacts of all named bodies; the contacts among them that
 *   hold a slot of the continuous-collision partition are given back by one lane in the loop's order, after a sort (a world
 *   without continuous collision has none). The contact array is compacted and the body-state table read back, as behind the
 *   single calls; a batch of b2hip_set_actives that only activates does neither. */
int b2hip_destroy_bodies(b2hip_world* w, int n, const int32_t* bodies);
/* active: one byte per entry, 0 = SetActive(false), non-zero = SetActive(true) */
int b2hip_set_actives(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* active);

/* ---- J. Batched fixture sets on the device (csrc/b2hip_api_fixture_batch.h, csrc/b2d_kernels_fixture_batch.h) ------------------
 * Change what many fixtures collide with, whether they are sensors or thick shapes, and their surface between two steps in
 * one call: a team goes ghost, debris stops colliding with debris, triggers are armed, a patch of ground turns to ice. The
 * single calls queue five small blocking copies per fixture for the next step, b2hip_fixture_set_filter / _sensor / _thick
 * also one or two contact-array operations per fixture, each of which is a walk of ONE workgroup over the whole contact
 * array, and b2hip_fixture_set_sensor wakes the body through the host's mirror (eight rows uploaded); these calls write the
 * proxies' words in one launch and visit the contact array once per call. They are four more write calls of block F's family
 * and follow the conventions of blocks H and I unless stated otherwise.
 *
 * Definition by equivalence. A call has the effect of the single call made for i = 0 .. n-1 in order with nothing in between:
 *   b2hip_fixture_set_filters:   b2hip_fixture_set_filter(w, fixtures[i], filters[i].category_bits, filters[i].mask_bits,
 *                                filters[i].group_index)
 *   b2hip_fixture_set_sensors:   b2hip_fixture_set_sensor(w, fixtures[i], sensor[i] != 0)
 *   b2hip_fixture_set_thicks:    b2hip_fixture_set_thick(w, fixtures[i], thick[i] != 0)
 *   b2hip_fixture_set_materials: b2hip_fixture_set_material(w, fixtures[i], density, friction, restitution) with each of the
 *                                three taken from materials[i] when its bit of `mask` is set, else the value the fixture has now
 * to the bit, for everything a caller can observe afterwards: b2hip_get_body_states / _of with awake bits and sleep times,
 * b2hip_get_contacts before and after later steps, the contact events of the next steps, b2hip_get_fat_aabb(s), batched
 * queries made before the next step (their filters read the proxies' words), a snapshot that is saved (it carries the
 * continuous-collision partition and the buffered moves), later single-fixture calls on the same fixtures, every later step
 * with continuous collision on.
 *   A sensor or thick entry that has the requested value already is a no-op, as the single call is: no wake, no contact is
 *   looked at. A filter entry always re-filters, as the single call does: every contact of the fixture is flagged for the next
 *   step's filter - a user contact filter (b2hip_set_contact_filter) is asked about it - and the proxy of a fixture whose body
 *   is active is buffered as moved, so that pairs the new filter admits can form. b2hip_fixture_set_sensors wakes the body of
 *   every entry that CHANGES (awake bit set, sleep time zero; a static body that is awake already is left untouched);
 *   b2hip_fixture_set_thicks wakes nobody. Sensors and thick shapes decide which contacts are candidates for continuous
 *   collision: the slots of that partition are appended and given back in the order the loop of single calls would have
 *   taken - by entry, within an entry newest contact first. b2hip_fixture_set_materials writes the proxies' friction and
 *   restitution for the contacts created from now on; existing contacts keep their mixture, and the density is read by the
 *   next mass computation only (no b2Body::ResetMassData is implied), as with the single call.
 * Order: edits made before the call lie underneath it: they go to the device first, queued contact operations of single calls
 *   included (block I says what that means for single calls mixed with batches), and edits made after it on top of it. Two
 *   calls before one step act one after the other.
 * fixtures: n fixture ids, each in [0, b2hip_fixture_count), not destroyed, and each AT MOST ONCE per call. A fixture of an
 *   inactive body can be named (it has no proxy: nothing is buffered for it).
 * Refusals, in this order: n outside [0, 2^24], a NULL fixtures / filters / sensor / thick / materials with n > 0:
 *   B2HIP_ERR_INVALID before the world is looked at. A NULL, failed or mid-step world (a listener's callback window
 *   included): B2HIP_ERR_INVALID. A sharded world: B2HIP_ERR_UNSUPPORTED. A mask that is 0 or has a bit beyond the three
 *   B2HIP_MATERIAL_* bits; an id out of range, a destroyed fixture or an id that occurs twice: B2HIP_ERR_INVALID, and
 *   b2hip_last_error names the first offender by entry and id. A refused call applies nothing. n == 0 is a successful no-op.
 *   A B2HIP_ERR_HIP from these calls is no refusal: a copy, a launch or a sort failed behind the host's bookkeeping, the device
 *   is partly edited, and the world is marked failed - every later call says so, and it can only be inspected and destroyed.
 * One refusal more, of b2hip_fixture_set_filters, checked before anything is written:
 *   The move buffer. The call adds its entries whose body is active to the moves the device has buffered, and if the sum does
 *     not fit (2 x fixtures + 64 entries, emptied by the step) it returns B2HIP_ERR_UNSUPPORTED, says to step first, and applies
 *     nothing. One batch over every fixture of a freshly stepped world always fits.
 * Cost: 4 + 16 bytes per entry cross in one copy; the device's counters (about 2 KB) come back first, and again at the end of
 *   every call but b2hip_fixture_set_materials, which launches once and reads nothing. The others pass over the contact array
 *   once, grid-wide. b2hip_fixture_set_sensors / _thicks then list the contacts whose candidacy for continuous collision
 *   changes - four bytes come back: the length - sort the list, and one lane replays it (a world without continuous collision
 *   lists nothing). b2hip_fixture_set_sensors reads the body-state table first if a batched write or a lazy world has left
 *   it on the device, as the single call does.
 * Out of scope: sharded worlds; calls inside a step or a listener callback; fixture creation and destruction; the drop-in C++
 *   classes (b2Fixture's setters bind the single calls). b2Body::SetType, SetBullet and ResetMassData for many bodies live in
 *   block K. */
typedef struct b2hip_fixture_filter
{
	uint16_t category_bits, mask_bits;
	int16_t  group_index;
	uint16_t pad;        /* 0 */
} b2hip_fixture_filter;
typedef struct b2hip_fixture_material
{
	float density, friction, restitution;
} b2hip_fixture_material;
#define B2HIP_MATERIAL_DENSITY 1
#define B2HIP_MATERIAL_FRICTION 2
#define B2HIP_MATERIAL_RESTITUTION 4

int b2hip_fixture_set_filters(b2hip_world* w, int n, const int32_t* fixtures, const b2hip_fixture_filter* filters);
/* sensor / thick: one byte per entry, 0 = false, non-zero = true */
int b2hip_fixture_set_sensors(b2hip_world* w, int n, const int32_t* fixtures, const uint8_t* sensor);
int b2hip_fixture_set_thicks(b2hip_world* w, int n, const int32_t* fixtures, const uint8_t* thick);
/* mask: a non-empty subset of B2HIP_MATERIAL_DENSITY | B2HIP_MATERIAL_FRICTION | B2HIP_MATERIAL_RESTITUTION */
int b2hip_fixture_set_materials(b2hip_world* w, int n, const int32_t* fixtures, const b2hip_fixture_material* materials, int mask);

/* ---- K. Batched body property sets on the device (csrc/b2hip_api_body_props.h, csrc/b2d_kernels_body_props.h) ----------------
 * Change the type, the bullet flag, the fixed-rotation flag, the permission to sleep, the damping and the mass data of many
 * bodies between two steps in one call: debris is frozen to static and thawed again, continuous collision is switched on for
 * everything that was just launched, a region gets drag, rotations are pinned, bodies are weighed again after
 * b2hip_fixture_set_materials changed their fixtures' densities (which implies no b2Body::ResetMassData). The single calls go
 * through the host's mirror - eight rows per run of consecutive ids uploaded with blocking copies by the next step - and
 * b2hip_set_type and b2hip_set_bullet queue one contact-array operation per body, each of which is a walk of ONE workgroup
 * over the whole contact array; these calls edit the bodies' rows in one launch and visit the contact array once per call. They
 * are seven more write calls of block F's family and follow the conventions of blocks H, I and J unless stated otherwise.
 *
 * Definition by equivalence. A call has the effect of the single call made for i = 0 .. n-1 in order with nothing in between:
 *   b2hip_set_types:             b2hip_set_type(w, bodies[i], type[i])
 *   b2hip_set_bullets:           b2hip_set_bullet(w, bodies[i], bullet[i] != 0)
 *   b2hip_set_fixed_rotations:   b2hip_set_fixed_rotation(w, bodies[i], flag[i] != 0)
 *   b2hip_set_sleeping_alloweds: b2hip_set_sleeping_allowed(w, bodies[i], flag[i] != 0)
 *   b2hip_set_body_dampings:     b2hip_set_body_damping(w, bodies[i], linear_damping, angular_damping, gravity_scale) with each
 *                                of the three taken from d[i] when its bit of `mask` is set, else the value the body has now
 *   b2hip_set_mass_datas:        b2hip_set_mass_data(w, bodies[i], &md[i])  (mass, inertia and local_center are read)
 *   b2hip_reset_mass_datas:      b2hip_set_mass_data(w, bodies[i], NULL)    (b2Body::ResetMassData)
 * to the bit, for everything a caller can observe afterwards: b2hip_get_body_states / _of with awake bits and sleep times,
 * b2hip_get_mass_data of every body, b2hip_get_contacts before and after later steps, the contact events, b2hip_get_fat_aabb(s),
 * b2hip_get_island_labels, a snapshot that is saved before the next step (it carries the sweep origins, the
 * continuous-collision partition and the buffered moves), later single calls on the same bodies, every later step with
 * continuous collision on.
 *   No-ops. An entry of b2hip_set_types whose body has the requested type already, of b2hip_set_fixed_rotations whose body has
 *   the requested flag already and of b2hip_set_bullets whose body has the requested flag already takes no part, as the single
 *   call changes nothing: no wake, no contact is looked at, no move is buffered. b2hip_set_mass_datas leaves a body that is not
 *   dynamic alone; a mass that is not positive becomes 1, and the inertia is taken only if it is positive and the body's
 *   rotation is not fixed. b2hip_reset_mass_datas gives a static or kinematic body zero mass and its origin as centre.
 *   Who wakes. b2hip_set_types wakes every body whose type changes - awake bit set, sleep time zero, force row zero, for a
 *   body that turns static too, whose velocity is zeroed as well - destroys every contact of every such body (a touching
 *   contact ends with an event and wakes the other body) and buffers every proxy of such a body that is active as moved,
 *   newest fixture first within a body, bodies in entry order, so that the next step finds its pairs again.
 *   b2hip_set_sleeping_alloweds wakes the body of every entry whose flag is 0 - awake bit set, sleep time zero, whether or not
 *   it slept - and nobody for a flag that is not 0. b2hip_set_bullets, b2hip_set_fixed_rotations, b2hip_set_body_dampings,
 *   b2hip_set_mass_datas and b2hip_reset_mass_datas wake nobody. b2hip_set_fixed_rotations zeroes the angular velocity of
 *   every body that changes; it and the mass-data calls move the centre of mass with the local centre
 *   (c = xf * local_center, v += cross(w, c - old c)) and the sweep origin with it, which a step with continuous collision
 *   sees. b2hip_set_bullets decides which contacts are candidates for continuous collision: the slots of that partition are
 *   appended and given back in the order the loop of single calls would have taken - by entry, within an entry newest contact
 *   first. A mouse joint reads its body's mass at the next step, as after the single calls.
 * Order: edits made before the call lie underneath it: they go to the device first, queued contact operations of single calls
 *   included (block I says what that means for single calls mixed with batches), and edits made after it on top of it. Two
 *   calls before one step act one after the other.
 * bodies: n body ids, each in [0, b2hip_body_count), not destroyed, and each AT MOST ONCE per call. An inactive body can be
 *   named (it has no proxies: nothing is buffered for it; its rows, its mass and its place in the seed order change). Bodies
 *   with joints take part like any other: the single calls do nothing joint-specific.
 * Refusals, in this order: n outside [0, 2^24], a NULL bodies / type / bullet / flag / d / md with n > 0: B2HIP_ERR_INVALID
 *   before the world is looked at. A NULL, failed or mid-step world (a listener's callback window included):
 *   B2HIP_ERR_INVALID. A sharded world: B2HIP_ERR_UNSUPPORTED. A mask that is 0 or has a bit beyond the three B2HIP_DAMPING_*
 *   bits, a type value above B2HIP_DYNAMIC_BODY; then an id out of range, a destroyed body or an id that occurs twice:
 *   B2HIP_ERR_INVALID, and b2hip_last_error names the first offender by entry and id. A refused call applies nothing. n == 0 is
 *   a successful no-op. A B2HIP_ERR_HIP from these calls is no refusal: a copy, a launch or a sort failed behind the host's
 *   bookkeeping, the device is partly edited, and the world is marked failed - every later call says so, and it can only be
 *   inspected and destroyed.
 * One refusal more, of b2hip_set_types, checked before anything is written:
 *   The move buffer. The call adds every proxy of its changing active bodies to the moves the device has buffered, and if the
 *     sum does not fit (2 x fixtures + 64 entries, emptied by the step) it returns B2HIP_ERR_UNSUPPORTED, says to step first,
 *     and applies nothing. One batch over every body of a freshly stepped world always fits.
 * The to-static refit fall-back. A body that turns static synchronises its fixtures with zero displacement
 *   (b2DynamicTree::MoveProxy): a proxy whose fat AABB no longer holds its shape's box would get a new one and a second move.
 *   After a step, and behind flushed teleports, every fat AABB holds its shape's box, so this is believed unreachable; the call
 *   tests it on the device all the same (one small launch over the proxies of the bodies that turn static, four bytes back),
 *   and a batch for which it is not so runs as the loop of single calls between the pending edits and the application of what
 *   the loop queued, as b2hip_destroy_bodies treats a batch with a jointed body. b2hip_debug_read 32 counts such batches.
 * Cost: 4 bytes per entry and 1 (flags), 16 (dampings) or 32 (fixed rotations, mass data, types; b2hip_set_types also 8 per
 *   moved proxy) cross in one copy; the device's counters (about 2 KB) come back first. b2hip_set_body_dampings,
 *   b2hip_set_sleeping_alloweds, b2hip_set_fixed_rotations and the mass-data calls launch once and read nothing more.
 *   b2hip_set_bullets passes over the contact array once, grid-wide, lists the contacts whose candidacy changes - four bytes
 *   come back: the length; a list longer than its room is listed again - sorts the list, and one lane replays it.
 *   b2hip_set_types passes over the contact array once and ends as b2hip_destroy_bodies does: the array is compacted and the
 *   body-state table read back.
 * Out of scope: sharded worlds; calls inside a step or a listener callback; the drop-in C++ classes (b2Body's setters bind the
 *   single calls). */
#define B2HIP_DAMPING_LINEAR 1
#define B2HIP_DAMPING_ANGULAR 2
#define B2HIP_DAMPING_GRAVITY_SCALE 4
typedef struct b2hip_body_damping
{
	float linear_damping, angular_damping, gravity_scale;
	float pad;           /* 0 */
} b2hip_body_damping;

/* type: one byte per entry, B2HIP_STATIC_BODY / B2HIP_KINEMATIC_BODY / B2HIP_DYNAMIC_BODY */
int b2hip_set_types(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* type);
/* bullet / flag: one byte per entry, 0 = false, non-zero = true */
int b2hip_set_bullets(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* bullet);
int b2hip_set_fixed_rotations(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* flag);
int b2hip_set_sleeping_alloweds(b2hip_world* w, int n, const int32_t* bodies, const uint8_t* flag);
/* mask: a non-empty subset of B2HIP_DAMPING_LINEAR | B2HIP_DAMPING_ANGULAR | B2HIP_DAMPING_GRAVITY_SCALE */
int b2hip_set_body_dampings(b2hip_world* w, int n, const int32_t* bodies, const b2hip_body_damping* d, int mask);
/* md: mass, inertia (about the local origin) and local_center are read; inv_mass and inv_inertia are not */
int b2hip_set_mass_datas(b2hip_world* w, int n, const int32_t* bodies, const b2hip_mass_data* md);
int b2hip_reset_mass_datas(b2hip_world* w, int n, const int32_t* bodies);

#ifdef __cplusplus
}
#endif

#endif
