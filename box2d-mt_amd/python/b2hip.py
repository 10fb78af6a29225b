"""ctypes binding of include/b2hip.h (libb2hip.so).

Plumbing only: every call goes straight to the C ABI; there is no Python or CPU implementation of the
step behind it.  Loading fails loudly if the HIP library is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libb2hip.so")

STATIC, KINEMATIC, DYNAMIC = 0, 1, 2
CIRCLE, EDGE, POLYGON = 0, 1, 2
POLYGON_RADIUS = np.float32(2.0) * np.float32(0.005)


class WorldDef(C.Structure):
    _fields_ = [("gravity_x", C.c_float), ("gravity_y", C.c_float), ("allow_sleep", C.c_int),
                ("warm_starting", C.c_int), ("continuous", C.c_int), ("sub_stepping", C.c_int),
                ("auto_clear_forces", C.c_int), ("device", C.c_int)]


class BodyDef(C.Structure):
    _fields_ = [("type", C.c_int), ("px", C.c_float), ("py", C.c_float), ("angle", C.c_float),
                ("vx", C.c_float), ("vy", C.c_float), ("w", C.c_float),
                ("linear_damping", C.c_float), ("angular_damping", C.c_float), ("gravity_scale", C.c_float),
                ("allow_sleep", C.c_int), ("awake", C.c_int), ("fixed_rotation", C.c_int),
                ("bullet", C.c_int), ("active", C.c_int)]


class Shape(C.Structure):
    _fields_ = [("type", C.c_int32), ("count", C.c_int32), ("radius", C.c_float), ("pad", C.c_float),
                ("centroid", C.c_float * 2), ("verts", C.c_float * 16), ("normals", C.c_float * 16)]


class FixtureDef(C.Structure):
    _fields_ = [("density", C.c_float), ("friction", C.c_float), ("restitution", C.c_float),
                ("category_bits", C.c_uint16), ("mask_bits", C.c_uint16), ("group_index", C.c_int16),
                ("pad", C.c_int16), ("is_sensor", C.c_int), ("thick_shape", C.c_int)]


class RevoluteJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("reference_angle", C.c_float), ("enable_limit", C.c_int),
                ("lower_angle", C.c_float), ("upper_angle", C.c_float), ("enable_motor", C.c_int),
                ("motor_speed", C.c_float), ("max_motor_torque", C.c_float), ("collide_connected", C.c_int)]


class DistanceJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("length", C.c_float), ("frequency_hz", C.c_float),
                ("damping_ratio", C.c_float), ("collide_connected", C.c_int)]


class PrismaticJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("local_axis_a", C.c_float * 2), ("reference_angle", C.c_float),
                ("enable_limit", C.c_int), ("lower_translation", C.c_float), ("upper_translation", C.c_float),
                ("enable_motor", C.c_int), ("motor_speed", C.c_float), ("max_motor_force", C.c_float),
                ("collide_connected", C.c_int)]


class WeldJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("reference_angle", C.c_float), ("frequency_hz", C.c_float),
                ("damping_ratio", C.c_float), ("collide_connected", C.c_int)]


class WheelJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("local_axis_a", C.c_float * 2), ("frequency_hz", C.c_float),
                ("damping_ratio", C.c_float), ("enable_motor", C.c_int), ("motor_speed", C.c_float),
                ("max_motor_torque", C.c_float), ("collide_connected", C.c_int)]


class RopeJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("max_length", C.c_float), ("collide_connected", C.c_int)]


class FrictionJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("local_anchor_a", C.c_float * 2),
                ("local_anchor_b", C.c_float * 2), ("max_force", C.c_float), ("max_torque", C.c_float),
                ("collide_connected", C.c_int)]


class MotorJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("linear_offset", C.c_float * 2), ("angular_offset", C.c_float),
                ("max_force", C.c_float), ("max_torque", C.c_float), ("correction_factor", C.c_float),
                ("collide_connected", C.c_int)]


class PulleyJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("ground_anchor_a", C.c_float * 2), ("ground_anchor_b", C.c_float * 2),
                ("local_anchor_a", C.c_float * 2), ("local_anchor_b", C.c_float * 2), ("length_a", C.c_float),
                ("length_b", C.c_float), ("ratio", C.c_float), ("collide_connected", C.c_int)]


class MouseJointDef(C.Structure):
    _fields_ = [("body_a", C.c_int), ("body_b", C.c_int), ("target", C.c_float * 2), ("max_force", C.c_float),
                ("frequency_hz", C.c_float), ("damping_ratio", C.c_float), ("collide_connected", C.c_int)]


class GearJointDef(C.Structure):
    _fields_ = [("joint1", C.c_int), ("joint2", C.c_int), ("ratio", C.c_float), ("collide_connected", C.c_int)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "bodies", "proxies", "contacts", "touching_contacts", "islands", "small_islands", "large_islands",
        "small_island_bodies", "small_island_contacts", "large_island_bodies", "large_island_contacts",
        "colors", "moved_proxies", "new_contacts", "destroyed_contacts", "solver_chunks",
        "pos_iterations_large", "overflow_flags", "toi_events", "toi_calls", "toi_pending_first_pass", "toi_serial_fallbacks",
        "blocks", "cut_constraints", "block_max_rows", "partitions", "block_solver_steps", "free_islands", "sweep_solver_steps",
        "hub_constraints", "hub_fixpoint_rounds", "hub_serial_chunks", "toi_chain_contacts", "toi_pre_solve_reruns", "solver_recoveries")]


BODY_STATE_DTYPE = np.dtype([("px", "f4"), ("py", "f4"), ("angle", "f4"), ("vx", "f4"), ("vy", "f4"), ("w", "f4"),
                             ("cx", "f4"), ("cy", "f4"), ("flags", "u4"), ("sleep_time", "f4")])

CONTACT_DTYPE = np.dtype([("fixture_a", "i4"), ("fixture_b", "i4"), ("body_a", "i4"), ("body_b", "i4"),
                          ("flags", "u4"), ("manifold_type", "i4"), ("point_count", "i4"),
                          ("local_normal", "f4", 2), ("local_point", "f4", 2), ("point_local", "f4", (2, 2)),
                          ("normal_impulse", "f4", 2), ("tangent_impulse", "f4", 2), ("id_key", "u4", 2),
                          ("friction", "f4"), ("restitution", "f4"), ("tangent_speed", "f4")])

class QueryFilter(C.Structure):
    _fields_ = [("mask", C.c_uint16), ("include_sensors", C.c_int)]


QUERY_ITEM_DTYPE = np.dtype([("fixture", "i4"), ("body", "i4")])
RAY_HIT_DTYPE = np.dtype([("fixture", "i4"), ("body", "i4"), ("point", "f4", 2), ("normal", "f4", 2), ("fraction", "f4"),
                          ("pad", "i4")])
SHAPE_QUERY_DTYPE = np.dtype([("shape", "i4"), ("x", "f4"), ("y", "f4"), ("angle", "f4")])
SHAPE_CAST_DTYPE = np.dtype([("shape", "i4"), ("x", "f4"), ("y", "f4"), ("angle", "f4"), ("tx", "f4"), ("ty", "f4"),
                             ("pad", "i4", 2)])
SHAPE_RANGE_DTYPE = np.dtype([("shape", "i4"), ("x", "f4"), ("y", "f4"), ("angle", "f4"), ("max_distance", "f4"), ("pad", "i4")])
DISTANCE_HIT_DTYPE = np.dtype([("fixture", "i4"), ("body", "i4"), ("point_a", "f4", 2), ("point_b", "f4", 2), ("distance", "f4"),
                               ("iterations", "i4")])
BODY_CONTACT_DTYPE = np.dtype([("contact_index", "i4"), ("other_body", "i4"), ("fixture", "i4"), ("other_fixture", "i4"),
                               ("normal", "f4", 2), ("normal_impulse", "f4"), ("tangent_impulse", "f4")])
BODY_CONTACT_TOTAL_DTYPE = np.dtype([("contacts", "i4"), ("touching", "i4"), ("impulse", "f4", 2), ("normal_impulse", "f4"),
                                     ("max_normal_impulse", "f4"), ("points", "i4"), ("pad", "i4")])
BODY_PUSH_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("angular", "f4"), ("at_point", "i4"), ("px", "f4"), ("py", "f4"),
                            ("pad", "i4", 2)])
JOINT_MOTOR_DTYPE = np.dtype([("enable_motor", "i4"), ("motor_speed", "f4"), ("max_motor", "f4"), ("pad", "i4")])
JOINT_STATE_DTYPE = np.dtype([("type", "i4"), ("limit_state", "i4"), ("coordinate", "f4"), ("speed", "f4"), ("coordinate2", "f4"),
                              ("speed2", "f4"), ("force", "f4", 2), ("torque", "f4"), ("motor", "f4"), ("pad", "f4", 2)])
JOINT_MOTOR_ENABLE, JOINT_MOTOR_SPEED, JOINT_MOTOR_MAX = 1, 2, 4  # the mask bits of b2hip_joint_set_motors
FIXTURE_FILTER_DTYPE = np.dtype([("category_bits", "u2"), ("mask_bits", "u2"), ("group_index", "i2"), ("pad", "u2")])
FIXTURE_MATERIAL_DTYPE = np.dtype([("density", "f4"), ("friction", "f4"), ("restitution", "f4")])
MATERIAL_DENSITY, MATERIAL_FRICTION, MATERIAL_RESTITUTION = 1, 2, 4  # the mask bits of b2hip_fixture_set_materials
BODY_DAMPING_DTYPE = np.dtype([("linear_damping", "f4"), ("angular_damping", "f4"), ("gravity_scale", "f4"), ("pad", "f4")])
DAMPING_LINEAR, DAMPING_ANGULAR, DAMPING_GRAVITY_SCALE = 1, 2, 4  # the mask bits of b2hip_set_body_dampings
MASS_DATA_DTYPE = np.dtype([("mass", "f4"), ("inertia", "f4"), ("local_center", "f4", 2), ("inv_mass", "f4"), ("inv_inertia", "f4")])

_lib = None


def _configure(L, optional_ok=False):
    """Declares the C-ABI signatures on a loaded library. `optional_ok`: the library may lack the measurement / phase
    entry points (the oracle's ABI shim used by the tests exports the world-building and stepping calls only)."""
    L.b2hip_last_error.restype = C.c_char_p
    L.b2hip_version.restype = C.c_char_p
    sigs = {
        "b2hip_world_create": [C.POINTER(WorldDef), C.POINTER(C.c_void_p)],
        "b2hip_world_destroy": [C.c_void_p],
        "b2hip_set_gravity": [C.c_void_p, C.c_float, C.c_float],
        "b2hip_shift_origin": [C.c_void_p, C.c_float, C.c_float],
        "b2hip_set_body_damping": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float],
        "b2hip_fixture_set_material": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float],
        "b2hip_set_flags": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int],
        "b2hip_create_body": [C.c_void_p, C.POINTER(BodyDef)],
        "b2hip_create_fixture": [C.c_void_p, C.c_int, C.POINTER(FixtureDef), C.POINTER(Shape)],
        "b2hip_create_revolute_joint": [C.c_void_p, C.POINTER(RevoluteJointDef)],
        "b2hip_create_distance_joint": [C.c_void_p, C.POINTER(DistanceJointDef)],
        "b2hip_create_prismatic_joint": [C.c_void_p, C.POINTER(PrismaticJointDef)],
        "b2hip_create_weld_joint": [C.c_void_p, C.POINTER(WeldJointDef)],
        "b2hip_create_wheel_joint": [C.c_void_p, C.POINTER(WheelJointDef)],
        "b2hip_create_rope_joint": [C.c_void_p, C.POINTER(RopeJointDef)],
        "b2hip_create_friction_joint": [C.c_void_p, C.POINTER(FrictionJointDef)],
        "b2hip_create_motor_joint": [C.c_void_p, C.POINTER(MotorJointDef)],
        "b2hip_create_pulley_joint": [C.c_void_p, C.POINTER(PulleyJointDef)],
        "b2hip_create_mouse_joint": [C.c_void_p, C.POINTER(MouseJointDef)],
        "b2hip_create_gear_joint": [C.c_void_p, C.POINTER(GearJointDef)],
        "b2hip_destroy_joint": [C.c_void_p, C.c_int],
        "b2hip_joint_set_target": [C.c_void_p, C.c_int, C.c_float, C.c_float],
        "b2hip_joint_set_offsets": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float],
        "b2hip_joint_set_motor": [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float],
        "b2hip_joint_set_limits": [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float],
        "b2hip_body_count": [C.c_void_p],
        "b2hip_fixture_count": [C.c_void_p],
        "b2hip_step": [C.c_void_p, C.c_float, C.c_int, C.c_int],
        "b2hip_step_begin": [C.c_void_p, C.c_float, C.c_int, C.c_int],
        "b2hip_collide": [C.c_void_p], "b2hip_solve": [C.c_void_p], "b2hip_sync_fixtures": [C.c_void_p],
        "b2hip_find_new_contacts": [C.c_void_p], "b2hip_solve_toi": [C.c_void_p], "b2hip_step_end": [C.c_void_p],
        "b2hip_get_body_states": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
        "b2hip_contact_count": [C.c_void_p],
        "b2hip_get_contacts": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_save_snapshot": [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
        "b2hip_load_snapshot": [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)],
        "b2hip_enable_contact_events": [C.c_void_p, C.c_int],
        "b2hip_get_contact_events": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_get_island_labels": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_get_fat_aabb": [C.c_void_p, C.c_int, C.POINTER(C.c_float)],
        "b2hip_get_fat_aabbs": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
        "b2hip_get_profile": [C.c_void_p, C.POINTER(C.c_float)],
        "b2hip_get_counters": [C.c_void_p, C.POINTER(Counters)],
        "b2hip_get_solver_timing": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "b2hip_apply_force": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int],
        "b2hip_set_velocity": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float],
        "b2hip_destroy_body": [C.c_void_p, C.c_int],
        "b2hip_destroy_fixture": [C.c_void_p, C.c_int],
        "b2hip_set_bullet": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_set_awake": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_fixture_set_sensor": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_fixture_refilter": [C.c_void_p, C.c_int],
        "b2hip_set_lazy_readback": [C.c_void_p, C.c_int],
        "b2hip_query_aabbs": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_query_points": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_ray_cast_closest": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_void_p],
        "b2hip_ray_cast_all": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_ray_cast_any": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_void_p],
        "b2hip_query_shapes": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_int,
                               C.c_void_p, C.c_void_p],
        "b2hip_shape_cast_closest": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter),
                                     C.c_void_p],
        "b2hip_shape_distance_closest": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter),
                                         C.c_void_p],
        "b2hip_query_shapes_within": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(QueryFilter), C.c_int,
                                      C.c_void_p, C.c_void_p],
        "b2hip_body_contacts": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_body_contact_totals": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_apply_linear_impulse": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int],
        "b2hip_apply_linear_impulse_to_center": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int],
        "b2hip_apply_angular_impulse": [C.c_void_p, C.c_int, C.c_float, C.c_int],
        "b2hip_apply_forces": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_apply_impulses": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_set_velocities": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_get_body_states_of": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_set_transform": [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float],
        "b2hip_set_transforms": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_set_awakes": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_set_active": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_destroy_bodies": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_set_actives": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_fixture_set_thick": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_fixture_set_filter": [C.c_void_p, C.c_int, C.c_uint16, C.c_uint16, C.c_int16],
        "b2hip_fixture_set_filters": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_fixture_set_sensors": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_fixture_set_thicks": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_fixture_set_materials": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_set_type": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_set_fixed_rotation": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_set_sleeping_allowed": [C.c_void_p, C.c_int, C.c_int],
        "b2hip_get_mass_data": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_set_mass_data": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_set_types": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_set_bullets": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_set_fixed_rotations": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_set_sleeping_alloweds": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_set_body_dampings": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_set_mass_datas": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
        "b2hip_reset_mass_datas": [C.c_void_p, C.c_int, C.c_void_p],
        "b2hip_get_joint_reaction": [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_float)],
        "b2hip_get_joint_limit_state": [C.c_void_p, C.c_int],
        "b2hip_joint_count": [C.c_void_p],
        "b2hip_joint_is_destroyed": [C.c_void_p, C.c_int],
        "b2hip_joint_set_motors": [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
        "b2hip_get_joint_states": [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p],
    }
    for name, argtypes in sigs.items():
        try:
            getattr(L, name).argtypes = argtypes
        except AttributeError:
            if not optional_ok:
                raise
    return L


def use_torch_hip_runtime():
    """Make torch's HIP runtime the one libb2hip.so binds to. torch ships its own libamdhip64 / libhsa-runtime64 and asks for
    them by another name, so a process that loads libb2hip.so first ends up with two HIP runtimes, and whichever of them opens
    the device second finds none (hipGetDeviceCount: no ROCm-capable device). With torch imported first, libb2hip.so's
    libamdhip64.so.7 resolves to torch's copy (same soname): one runtime. Call it before loading any library that links
    libb2hip.so."""
    try:
        import torch  # noqa: F401
    except ImportError:  # (no torch in the process: the system runtime is the only one)
        pass


def load(path, optional_ok=False):
    """Any library that exports the b2hip C ABI (the product, or the tests' oracle shim)."""
    use_torch_hip_runtime()
    return _configure(C.CDLL(path), optional_ok)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libb2hip.so is not built (%s): run __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
        _lib = load(LIB_PATH)
    return _lib


class B2HipError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise B2HipError("b2hip error %d: %s" % (rc, (_lib.b2hip_last_error().decode() if _lib is not None else "?")))
    return rc


def box_shape(hx, hy):
    s = Shape()
    s.type, s.count, s.radius = POLYGON, 4, POLYGON_RADIUS
    hx, hy = np.float32(hx), np.float32(hy)
    v = [-hx, -hy, hx, -hy, hx, hy, -hx, hy]
    n = [0, -1, 1, 0, 0, 1, -1, 0]
    for i in range(8):
        s.verts[i] = v[i]
        s.normals[i] = n[i]
    return s


def circle_shape(radius, px=0.0, py=0.0):
    s = Shape()
    s.type, s.count, s.radius = CIRCLE, 0, radius
    s.verts[0], s.verts[1] = px, py
    return s


def edge_shape(v1, v2):
    s = Shape()
    s.type, s.count, s.radius = EDGE, 0, POLYGON_RADIUS
    s.verts[0], s.verts[1], s.verts[2], s.verts[3] = v1[0], v1[1], v2[0], v2[1]
    return s


class World:
    def __init__(self, gravity=(0.0, -10.0), allow_sleep=True, warm_starting=True, continuous=False, device=-1, library=None):
        self.L = library if library is not None else lib()
        d = WorldDef(gravity[0], gravity[1], int(allow_sleep), int(warm_starting), int(continuous), 0, 1, device)
        p = C.c_void_p()
        _check(self.L.b2hip_world_create(C.byref(d), C.byref(p)))
        self.p = p

    def save_snapshot(self):
        """The world as bytes (b2hip_save_snapshot): bodies, fixtures, joints, contacts with warm-start state, counters."""
        need = C.c_size_t(0)
        _check(self.L.b2hip_save_snapshot(self.p, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        _check(self.L.b2hip_save_snapshot(self.p, buf, need.value, C.byref(need)))
        return buf.raw[:need.value]

    @classmethod
    def from_snapshot(cls, blob, device=-1, library=None):
        self = cls.__new__(cls)
        self.L = library if library is not None else lib()
        p = C.c_void_p()
        _check(self.L.b2hip_load_snapshot(blob, len(blob), device, C.byref(p)))
        self.p = p
        return self

    @classmethod
    def borrow(cls, ptr, library=None):
        """A view of a world owned elsewhere (the drop-in's b2World::GetDeviceWorld()): close() leaves the world alone."""
        self = cls.__new__(cls)
        self.L = library if library is not None else lib()
        self.p = C.c_void_p(ptr)
        self._borrowed = True
        return self

    def close(self):
        if self.p and not getattr(self, "_borrowed", False):
            self.L.b2hip_world_destroy(self.p)
        self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def create_body(self, type=STATIC, position=(0.0, 0.0), angle=0.0, velocity=(0.0, 0.0), omega=0.0,
                    linear_damping=0.0, angular_damping=0.0, gravity_scale=1.0, allow_sleep=True, awake=True,
                    fixed_rotation=False, bullet=False):
        d = BodyDef(type, position[0], position[1], angle, velocity[0], velocity[1], omega, linear_damping,
                    angular_damping, gravity_scale, int(allow_sleep), int(awake), int(fixed_rotation), int(bullet), 1)
        return _check(self.L.b2hip_create_body(self.p, C.byref(d)))

    def create_fixture(self, body, shape, density=0.0, friction=0.2, restitution=0.0, category=1, mask=0xFFFF,
                       group=0, sensor=False, thick=False):
        d = FixtureDef(density, friction, restitution, category, mask, group, 0, int(sensor), int(thick))
        return _check(self.L.b2hip_create_fixture(self.p, body, C.byref(d), C.byref(shape)))

    def create_revolute_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), reference_angle=0.0,
                              enable_limit=False, lower=0.0, upper=0.0, enable_motor=False, motor_speed=0.0,
                              max_motor_torque=0.0, collide_connected=False):
        d = RevoluteJointDef()
        d.body_a, d.body_b = body_a, body_b
        d.local_anchor_a[0], d.local_anchor_a[1] = anchor_a
        d.local_anchor_b[0], d.local_anchor_b[1] = anchor_b
        d.reference_angle = reference_angle
        d.enable_limit, d.lower_angle, d.upper_angle = int(enable_limit), lower, upper
        d.enable_motor, d.motor_speed, d.max_motor_torque = int(enable_motor), motor_speed, max_motor_torque
        d.collide_connected = int(collide_connected)
        return _check(self.L.b2hip_create_revolute_joint(self.p, C.byref(d)))

    def create_distance_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), length=1.0,
                              frequency_hz=0.0, damping_ratio=0.0, collide_connected=False):
        d = DistanceJointDef()
        d.body_a, d.body_b = body_a, body_b
        d.local_anchor_a[0], d.local_anchor_a[1] = anchor_a
        d.local_anchor_b[0], d.local_anchor_b[1] = anchor_b
        d.length, d.frequency_hz, d.damping_ratio = length, frequency_hz, damping_ratio
        d.collide_connected = int(collide_connected)
        return _check(self.L.b2hip_create_distance_joint(self.p, C.byref(d)))

    def create_prismatic_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), axis=(1.0, 0.0),
                               reference_angle=0.0, enable_limit=False, lower=0.0, upper=0.0, enable_motor=False,
                               motor_speed=0.0, max_motor_force=0.0, collide_connected=False):
        d = PrismaticJointDef()
        d.body_a, d.body_b = body_a, body_b
        d.local_anchor_a[0], d.local_anchor_a[1] = anchor_a
        d.local_anchor_b[0], d.local_anchor_b[1] = anchor_b
        d.local_axis_a[0], d.local_axis_a[1] = axis
        d.reference_angle = reference_angle
        d.enable_limit, d.lower_translation, d.upper_translation = int(enable_limit), lower, upper
        d.enable_motor, d.motor_speed, d.max_motor_force = int(enable_motor), motor_speed, max_motor_force
        d.collide_connected = int(collide_connected)
        return _check(self.L.b2hip_create_prismatic_joint(self.p, C.byref(d)))

    def create_weld_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), reference_angle=0.0,
                          frequency_hz=0.0, damping_ratio=0.0, collide_connected=False):
        d = WeldJointDef()
        d.body_a, d.body_b = body_a, body_b
        d.local_anchor_a[0], d.local_anchor_a[1] = anchor_a
        d.local_anchor_b[0], d.local_anchor_b[1] = anchor_b
        d.reference_angle, d.frequency_hz, d.damping_ratio = reference_angle, frequency_hz, damping_ratio
        d.collide_connected = int(collide_connected)
        return _check(self.L.b2hip_create_weld_joint(self.p, C.byref(d)))

    def _joint_def(self, cls, body_a, body_b, anchor_a, anchor_b, collide_connected):
        d = cls()
        d.body_a, d.body_b = body_a, body_b
        if anchor_a is not None:
            d.local_anchor_a[0], d.local_anchor_a[1] = anchor_a
            d.local_anchor_b[0], d.local_anchor_b[1] = anchor_b
        d.collide_connected = int(collide_connected)
        return d

    def create_wheel_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), axis=(1.0, 0.0), frequency_hz=2.0,
                           damping_ratio=0.7, enable_motor=False, motor_speed=0.0, max_motor_torque=0.0, collide_connected=False):
        d = self._joint_def(WheelJointDef, body_a, body_b, anchor_a, anchor_b, collide_connected)
        d.local_axis_a[0], d.local_axis_a[1] = axis
        d.frequency_hz, d.damping_ratio = frequency_hz, damping_ratio
        d.enable_motor, d.motor_speed, d.max_motor_torque = int(enable_motor), motor_speed, max_motor_torque
        return _check(self.L.b2hip_create_wheel_joint(self.p, C.byref(d)))

    def create_rope_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), max_length=1.0, collide_connected=False):
        d = self._joint_def(RopeJointDef, body_a, body_b, anchor_a, anchor_b, collide_connected)
        d.max_length = max_length
        return _check(self.L.b2hip_create_rope_joint(self.p, C.byref(d)))

    def create_friction_joint(self, body_a, body_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), max_force=0.0, max_torque=0.0,
                              collide_connected=False):
        d = self._joint_def(FrictionJointDef, body_a, body_b, anchor_a, anchor_b, collide_connected)
        d.max_force, d.max_torque = max_force, max_torque
        return _check(self.L.b2hip_create_friction_joint(self.p, C.byref(d)))

    def create_motor_joint(self, body_a, body_b, linear_offset=(0.0, 0.0), angular_offset=0.0, max_force=1.0, max_torque=1.0,
                           correction_factor=0.3, collide_connected=False):
        d = self._joint_def(MotorJointDef, body_a, body_b, None, None, collide_connected)
        d.linear_offset[0], d.linear_offset[1] = linear_offset
        d.angular_offset = angular_offset
        d.max_force, d.max_torque, d.correction_factor = max_force, max_torque, correction_factor
        return _check(self.L.b2hip_create_motor_joint(self.p, C.byref(d)))

    def create_pulley_joint(self, body_a, body_b, ground_a, ground_b, anchor_a=(0.0, 0.0), anchor_b=(0.0, 0.0), length_a=1.0,
                            length_b=1.0, ratio=1.0, collide_connected=True):
        d = self._joint_def(PulleyJointDef, body_a, body_b, anchor_a, anchor_b, collide_connected)
        d.ground_anchor_a[0], d.ground_anchor_a[1] = ground_a
        d.ground_anchor_b[0], d.ground_anchor_b[1] = ground_b
        d.length_a, d.length_b, d.ratio = length_a, length_b, ratio
        return _check(self.L.b2hip_create_pulley_joint(self.p, C.byref(d)))

    def create_mouse_joint(self, body_a, body_b, target, max_force, frequency_hz=5.0, damping_ratio=0.7, collide_connected=False):
        d = self._joint_def(MouseJointDef, body_a, body_b, None, None, collide_connected)
        d.target[0], d.target[1] = target
        d.max_force, d.frequency_hz, d.damping_ratio = max_force, frequency_hz, damping_ratio
        return _check(self.L.b2hip_create_mouse_joint(self.p, C.byref(d)))

    def create_gear_joint(self, joint1, joint2, ratio=1.0, collide_connected=False):
        d = GearJointDef(joint1, joint2, ratio, int(collide_connected))
        return _check(self.L.b2hip_create_gear_joint(self.p, C.byref(d)))

    def destroy_joint(self, joint):
        _check(self.L.b2hip_destroy_joint(self.p, joint))

    def destroy_body(self, body):
        """b2World::DestroyBody: the body, its fixtures, its joints and its contacts (ids are never reused)."""
        _check(self.L.b2hip_destroy_body(self.p, body))

    def destroy_fixture(self, fixture):
        _check(self.L.b2hip_destroy_fixture(self.p, fixture))

    def shift_origin(self, x, y):
        _check(self.L.b2hip_shift_origin(self.p, x, y))

    def set_bullet(self, body, flag=True):
        _check(self.L.b2hip_set_bullet(self.p, body, int(flag)))

    def set_type(self, body, type):
        """b2Body::SetType: STATIC, KINEMATIC or DYNAMIC; the body's contacts go, its mass data are computed again, it wakes."""
        _check(self.L.b2hip_set_type(self.p, body, int(type)))

    def set_body_damping(self, body, linear, angular, gravity_scale):
        """b2Body::SetLinearDamping / SetAngularDamping / SetGravityScale: read by the next step."""
        _check(self.L.b2hip_set_body_damping(self.p, body, linear, angular, gravity_scale))

    def set_fixed_rotation(self, body, flag=True):
        """b2Body::SetFixedRotation: the flag, no spin, mass data again."""
        _check(self.L.b2hip_set_fixed_rotation(self.p, body, int(flag)))

    def set_sleeping_allowed(self, body, flag=True):
        """b2Body::SetSleepingAllowed: a body that may not sleep is woken."""
        _check(self.L.b2hip_set_sleeping_allowed(self.p, body, int(flag)))

    def set_mass_data(self, body, mass=None, inertia=0.0, local_center=(0.0, 0.0)):
        """b2Body::SetMassData (inertia about the body's origin); mass None: b2Body::ResetMassData."""
        if mass is None:
            _check(self.L.b2hip_set_mass_data(self.p, body, None))
            return
        md = np.zeros(1, MASS_DATA_DTYPE)
        md["mass"], md["inertia"], md["local_center"] = mass, inertia, local_center
        _check(self.L.b2hip_set_mass_data(self.p, body, md.ctypes.data_as(C.c_void_p)))

    def mass_data(self, body):
        """b2hip_get_mass_data: one MASS_DATA_DTYPE record (mass, inertia about the origin, local centre, inverse mass and inertia)."""
        md = np.zeros(1, MASS_DATA_DTYPE)
        _check(self.L.b2hip_get_mass_data(self.p, body, md.ctypes.data_as(C.c_void_p)))
        return md[0]

    def set_awake(self, body, flag=True):
        _check(self.L.b2hip_set_awake(self.p, body, int(flag)))

    def set_active(self, body, flag=True):
        """b2Body::SetActive: an inactive body keeps its fixtures and its state, and has no proxies and no contacts."""
        _check(self.L.b2hip_set_active(self.p, body, int(flag)))

    def set_transform(self, body, position, angle):
        """b2Body::SetTransform: the body's origin and angle; it keeps its velocity and does not wake."""
        _check(self.L.b2hip_set_transform(self.p, body, position[0], position[1], angle))

    def fixture_set_sensor(self, fixture, flag=True):
        _check(self.L.b2hip_fixture_set_sensor(self.p, fixture, int(flag)))

    def fixture_refilter(self, fixture):
        _check(self.L.b2hip_fixture_refilter(self.p, fixture))

    def fixture_set_filter(self, fixture, category_bits, mask_bits, group_index=0):
        """b2Fixture::SetFilterData: the new filter, and the fixture's contacts re-filtered at the next step."""
        _check(self.L.b2hip_fixture_set_filter(self.p, fixture, category_bits, mask_bits, group_index))

    def fixture_set_thick(self, fixture, flag=True):
        _check(self.L.b2hip_fixture_set_thick(self.p, fixture, int(flag)))

    def fixture_set_material(self, fixture, density, friction, restitution):
        """b2Fixture::SetDensity / SetFriction / SetRestitution: for the next mass computation / the contacts created from now on."""
        _check(self.L.b2hip_fixture_set_material(self.p, fixture, density, friction, restitution))

    def joint_set_target(self, joint, target):
        _check(self.L.b2hip_joint_set_target(self.p, joint, target[0], target[1]))

    def joint_set_offsets(self, joint, linear_offset, angular_offset):
        _check(self.L.b2hip_joint_set_offsets(self.p, joint, linear_offset[0], linear_offset[1], angular_offset))

    def joint_set_motor(self, joint, enable_motor, motor_speed, max_motor):
        _check(self.L.b2hip_joint_set_motor(self.p, joint, int(enable_motor), motor_speed, max_motor))

    def joint_set_limits(self, joint, enable_limit, lower, upper):
        _check(self.L.b2hip_joint_set_limits(self.p, joint, int(enable_limit), lower, upper))

    def apply_force(self, body, force=(0.0, 0.0), torque=0.0, wake=True):
        _check(self.L.b2hip_apply_force(self.p, body, force[0], force[1], torque, int(wake)))

    def apply_linear_impulse(self, body, impulse, point, wake=True):
        _check(self.L.b2hip_apply_linear_impulse(self.p, body, impulse[0], impulse[1], point[0], point[1], int(wake)))

    def apply_linear_impulse_to_center(self, body, impulse, wake=True):
        _check(self.L.b2hip_apply_linear_impulse_to_center(self.p, body, impulse[0], impulse[1], int(wake)))

    def apply_angular_impulse(self, body, impulse, wake=True):
        _check(self.L.b2hip_apply_angular_impulse(self.p, body, impulse, int(wake)))

    def set_flags(self, allow_sleep=True, warm_starting=True, continuous=False, sub_stepping=False):
        _check(self.L.b2hip_set_flags(self.p, int(allow_sleep), int(warm_starting), int(continuous), int(sub_stepping)))

    def set_velocity(self, body, velocity=(0.0, 0.0), omega=0.0):
        _check(self.L.b2hip_set_velocity(self.p, body, velocity[0], velocity[1], omega))

    def set_lazy_readback(self, enable=True):
        """The 40 B per body of a step's read-back stay in HBM until body_states() (or an edit) asks for them."""
        _check(self.L.b2hip_set_lazy_readback(self.p, int(enable)))

    def step(self, dt=1.0 / 60.0, vel_iters=8, pos_iters=3):
        _check(self.L.b2hip_step(self.p, dt, vel_iters, pos_iters))

    @property
    def body_count(self):
        return self.L.b2hip_body_count(self.p)

    def body_states(self):
        n = self.body_count
        out = np.zeros(n, BODY_STATE_DTYPE)
        _check(self.L.b2hip_get_body_states(self.p, 0, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def bodies8(self):
        """Same 8-column layout as the harness: x, y, angle, vx, vy, w, awake, type."""
        s = self.body_states()
        out = np.zeros((s.size, 8), np.float32)
        out[:, 0], out[:, 1], out[:, 2] = s["px"], s["py"], s["angle"]
        out[:, 3], out[:, 4], out[:, 5] = s["vx"], s["vy"], s["w"]
        out[:, 6] = (s["flags"] & 4) != 0
        out[:, 7] = s["flags"] & 3
        return out

    @property
    def contact_count(self):
        return self.L.b2hip_contact_count(self.p)

    def contacts(self):
        cap = max(self.contact_count, 1)
        out = np.zeros(cap, CONTACT_DTYPE)
        n = _check(self.L.b2hip_get_contacts(self.p, cap, out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def enable_contact_events(self, enable=True):
        _check(self.L.b2hip_enable_contact_events(self.p, 1 if enable else 0))

    def contact_events(self):
        """Begin / end events of the last step: rows (fixture_a, fixture_b, kind 0 begin / 1 end, contact_index or -1)."""
        n = _check(self.L.b2hip_get_contact_events(self.p, 0, None))
        out = np.zeros((max(n, 1), 4), np.int32)
        n = _check(self.L.b2hip_get_contact_events(self.p, n, out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def island_labels(self):
        n = self.body_count
        out = np.zeros(n, np.int32)
        _check(self.L.b2hip_get_island_labels(self.p, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def counters(self):
        c = Counters()
        _check(self.L.b2hip_get_counters(self.p, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def profile(self):
        ms = (C.c_float * 13)()
        _check(self.L.b2hip_get_profile(self.p, ms))
        return list(ms)

    # ---- batched queries on the device (include/b2hip.h: b2hip_query_aabbs, b2hip_query_points, b2hip_ray_cast_closest / _all / _any)
    @staticmethod
    def _pairs(a, name):
        a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("%s: an (n, 2) array is expected, got shape %s" % (name, a.shape))
        return a

    def _query(self, fn, data, n, mask, sensors, lead=(), dtype=QUERY_ITEM_DTYPE):
        f = QueryFilter(mask, int(bool(sensors)))
        offsets = np.zeros(n + 1, np.int32)
        items = np.zeros(max(n, 1) * 8, dtype)
        for _ in range(2):  # (once more with the exact capacity when the first guess was short)
            total = _check(fn(self.p, *lead, n, data.ctypes.data_as(C.c_void_p), C.byref(f), items.size,
                              offsets.ctypes.data_as(C.c_void_p), items.ctypes.data_as(C.c_void_p)))
            if total <= items.size:
                return offsets, items[:total]
            items = np.zeros(total, dtype)
        raise B2HipError("query: the result grew between two identical calls")

    def query_aabbs(self, lower, upper, mask=0xFFFF, sensors=True):
        """Every fixture whose fat AABB overlaps box i = (lower[i], upper[i]): returns (offsets[n + 1], items) with
        items[offsets[i]:offsets[i + 1]] the (fixture, body) rows of box i in ascending fixture id."""
        lo, hi = self._pairs(lower, "lower"), self._pairs(upper, "upper")
        if lo.shape != hi.shape:
            raise ValueError("query_aabbs: lower and upper differ in shape")
        boxes = np.ascontiguousarray(np.concatenate([lo, hi], axis=1))
        return self._query(self.L.b2hip_query_aabbs, boxes, len(boxes), mask, sensors)

    def query_points(self, points, mask=0xFFFF, sensors=True):
        """The fixtures whose shape contains point i (b2Fixture::TestPoint within the fat AABB): (offsets, items) as query_aabbs."""
        pts = self._pairs(points, "points")
        return self._query(self.L.b2hip_query_points, pts, len(pts), mask, sensors)

    def _rays(self, p1, p2, name):
        a, b = self._pairs(p1, "p1"), self._pairs(p2, "p2")
        if a.shape != b.shape:
            raise ValueError("%s: p1 and p2 differ in shape" % name)
        return np.ascontiguousarray(np.concatenate([a, b], axis=1))

    def ray_cast_closest(self, p1, p2, mask=0xFFFF, sensors=True):
        """Closest hit of ray i from p1[i] to p2[i]: a RAY_HIT_DTYPE array, fixture = -1 where the ray hits nothing."""
        rays = self._rays(p1, p2, "ray_cast_closest")
        out = np.zeros(len(rays), RAY_HIT_DTYPE)
        f = QueryFilter(mask, int(bool(sensors)))
        _check(self.L.b2hip_ray_cast_closest(self.p, len(rays), rays.ctypes.data_as(C.c_void_p), C.byref(f),
                                             out.ctypes.data_as(C.c_void_p)))
        return out

    def ray_cast_all(self, p1, p2, mask=0xFFFF, sensors=True):
        """Every fixture ray i crosses from p1[i] to p2[i]: (offsets[n + 1], hits) with hits[offsets[i]:offsets[i + 1]] the
        RAY_HIT_DTYPE records of ray i in ascending (fraction, fixture id); the first is ray_cast_closest's."""
        rays = self._rays(p1, p2, "ray_cast_all")
        return self._query(self.L.b2hip_ray_cast_all, rays, len(rays), mask, sensors, dtype=RAY_HIT_DTYPE)

    def ray_cast_any(self, p1, p2, mask=0xFFFF, sensors=True):
        """Whether ray i from p1[i] to p2[i] crosses a fixture: a bool array of n (ray_cast_closest(...)["fixture"] >= 0)."""
        rays = self._rays(p1, p2, "ray_cast_any")
        out = np.zeros(len(rays), np.uint8)
        f = QueryFilter(mask, int(bool(sensors)))
        _check(self.L.b2hip_ray_cast_any(self.p, len(rays), rays.ctypes.data_as(C.c_void_p), C.byref(f),
                                         out.ctypes.data_as(C.c_void_p)))
        return out.astype(bool)

    @staticmethod
    def _shape_table(shapes, n, shape_index):
        """(Shape array, shape count, int32 index per query): one Shape serves every query, n Shapes default to one each"""
        one = isinstance(shapes, Shape)
        shapes = [shapes] if one else list(shapes)
        table = (Shape * max(len(shapes), 1))(*shapes)
        if shape_index is None:
            if not one and len(shapes) != n:
                raise ValueError("shape_index is needed when the number of shapes (%d) is not the number of queries (%d)"
                                 % (len(shapes), n))
            shape_index = np.zeros(n, np.int32) if one else np.arange(n, dtype=np.int32)
        shape_index = np.asarray(shape_index, np.int32).reshape(-1)
        if len(shape_index) != n:
            raise ValueError("shape_index: %d entries for %d queries" % (len(shape_index), n))
        return table, len(shapes), shape_index

    @staticmethod
    def _poses(poses):
        p = np.ascontiguousarray(poses, np.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("poses: an (n, 3) array of (x, y, angle) is expected, got shape %s" % (p.shape,))
        return p

    def query_shapes(self, shapes, poses, shape_index=None, mask=0xFFFF, sensors=True):
        """The fixtures a shape overlaps (b2TestOverlap) at pose i = (x, y, angle): (offsets, items) as query_aabbs.
        shapes: one Shape (every pose) or a list of them (shape_index picks one per pose; by default the i-th)."""
        p = self._poses(poses)
        table, ns, idx = self._shape_table(shapes, len(p), shape_index)
        q = np.zeros(len(p), SHAPE_QUERY_DTYPE)
        q["shape"] = idx
        q["x"], q["y"], q["angle"] = p[:, 0], p[:, 1], p[:, 2]
        return self._query(self.L.b2hip_query_shapes, q, len(q), mask, sensors, lead=(ns, C.cast(table, C.c_void_p)))

    def shape_cast_closest(self, shapes, poses, translations, shape_index=None, mask=0xFFFF, sensors=True):
        """The first fixture a shape meets moving from pose i by translation i (b2ShapeCast): a RAY_HIT_DTYPE array whose
        fraction is the cast's lambda; fixture = -1 where it meets nothing (fixtures it overlaps at the pose included)."""
        p = self._poses(poses)
        t = self._pairs(translations, "translations")
        if len(t) != len(p):
            raise ValueError("shape_cast_closest: %d poses, %d translations" % (len(p), len(t)))
        table, ns, idx = self._shape_table(shapes, len(p), shape_index)
        c = np.zeros(len(p), SHAPE_CAST_DTYPE)
        c["shape"] = idx
        c["x"], c["y"], c["angle"] = p[:, 0], p[:, 1], p[:, 2]
        c["tx"], c["ty"] = t[:, 0], t[:, 1]
        out = np.zeros(len(c), RAY_HIT_DTYPE)
        f = QueryFilter(mask, int(bool(sensors)))
        _check(self.L.b2hip_shape_cast_closest(self.p, ns, C.cast(table, C.c_void_p), len(c), c.ctypes.data_as(C.c_void_p),
                                               C.byref(f), out.ctypes.data_as(C.c_void_p)))
        return out

    @staticmethod
    def _ranges(shapes, poses, max_distance, shape_index):
        """(SHAPE_RANGE_DTYPE records, shape count, Shape array) of a distance batch"""
        p = World._poses(poses)
        table, ns, idx = World._shape_table(shapes, len(p), shape_index)
        r = np.zeros(len(p), SHAPE_RANGE_DTYPE)
        r["shape"] = idx
        r["x"], r["y"], r["angle"] = p[:, 0], p[:, 1], p[:, 2]
        d = np.asarray(max_distance, np.float32)
        if d.ndim > 1 or (d.ndim == 1 and len(d) != len(p)):
            raise ValueError("max_distance: a scalar or an (n,) array is expected, got shape %s for %d poses" % (d.shape, len(p)))
        r["max_distance"] = d
        return r, ns, table

    def shape_distance_closest(self, shapes, poses, max_distance, shape_index=None, mask=0xFFFF, sensors=True):
        """The nearest fixture within max_distance (a scalar or one per pose) of a shape at pose i = (x, y, angle), by
        b2Distance with the radii: a DISTANCE_HIT_DTYPE array with the distance and the closest points on the shape (point_a)
        and on the fixture (point_b); fixture = -1 and distance = inf where nothing is within range. 0 where they overlap."""
        r, ns, table = self._ranges(shapes, poses, max_distance, shape_index)
        out = np.zeros(len(r), DISTANCE_HIT_DTYPE)
        f = QueryFilter(mask, int(bool(sensors)))
        _check(self.L.b2hip_shape_distance_closest(self.p, ns, C.cast(table, C.c_void_p), len(r), r.ctypes.data_as(C.c_void_p),
                                                   C.byref(f), out.ctypes.data_as(C.c_void_p)))
        return out

    def query_shapes_within(self, shapes, poses, max_distance, shape_index=None, mask=0xFFFF, sensors=True):
        """Every fixture within max_distance of a shape at pose i: (offsets[n + 1], hits) with hits[offsets[i]:offsets[i + 1]]
        the DISTANCE_HIT_DTYPE records of pose i in ascending fixture id."""
        r, ns, table = self._ranges(shapes, poses, max_distance, shape_index)
        return self._query(self.L.b2hip_query_shapes_within, r, len(r), mask, sensors, lead=(ns, C.cast(table, C.c_void_p)),
                           dtype=DISTANCE_HIT_DTYPE)

    # ---- per-body contact lists and totals on the device (include/b2hip.h: b2hip_body_contacts, b2hip_body_contact_totals)
    @staticmethod
    def _body_ids(bodies):
        b = np.ascontiguousarray(bodies, np.int32)
        if b.ndim != 1:
            raise ValueError("bodies: an (n,) array of body ids is expected, got shape %s" % (b.shape,))
        return b

    def body_contacts(self, bodies, touching_only=True):
        """The contacts of each body of `bodies` (ids, each once): (offsets[n + 1], records) with
        records[offsets[i]:offsets[i + 1]] the BODY_CONTACT_DTYPE records of bodies[i] in ascending contact_index (an index into
        contacts() read at the same point); normal points from the other body towards this one."""
        b = self._body_ids(bodies)
        n = len(b)
        offsets = np.zeros(n + 1, np.int32)
        records = np.zeros(max(n, 1) * 8, BODY_CONTACT_DTYPE)
        for _ in range(2):  # (once more with the exact capacity when the first guess was short)
            total = _check(self.L.b2hip_body_contacts(self.p, n, b.ctypes.data_as(C.c_void_p), int(bool(touching_only)), records.size,
                                                      offsets.ctypes.data_as(C.c_void_p), records.ctypes.data_as(C.c_void_p)))
            if total <= records.size:
                return offsets, records[:total]
            records = np.zeros(total, BODY_CONTACT_DTYPE)
        raise B2HipError("body_contacts: the result grew between two identical calls")

    def body_contact_totals(self, bodies):
        """One BODY_CONTACT_TOTAL_DTYPE record per body of `bodies`: its contacts, how many touch, and over the touching ones
        the net impulse of the last step on the body (world frame), the sum and the largest of the normal impulses, the points."""
        b = self._body_ids(bodies)
        out = np.zeros(len(b), BODY_CONTACT_TOTAL_DTYPE)
        _check(self.L.b2hip_body_contact_totals(self.p, len(b), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- batched body writes on the device (include/b2hip.h, block F: b2hip_apply_forces, b2hip_apply_impulses,
    # b2hip_set_velocities, b2hip_get_body_states_of)
    @classmethod
    def _pushes(cls, n, linear, angular, point, name):
        """n BODY_PUSH_DTYPE records: `linear` (n, 2) or one pair, `angular` (n,) or one number, `point` None (at the centre
        of mass), (n, 2) or one pair."""
        push = np.zeros(n, BODY_PUSH_DTYPE)
        lin = np.asarray(linear, np.float32)
        lin = cls._pairs(np.broadcast_to(lin, (n, 2)) if lin.ndim == 1 and lin.shape == (2,) else lin, name)
        ang = np.asarray(angular, np.float32)
        if ang.ndim > 1 or (ang.ndim == 1 and len(ang) != n) or len(lin) != n:
            raise ValueError("%s: %d bodies, %d vectors, angular of shape %s" % (name, n, len(lin), ang.shape))
        push["x"], push["y"], push["angular"] = lin[:, 0], lin[:, 1], ang
        if point is not None:
            pt = np.asarray(point, np.float32)
            pt = cls._pairs(np.broadcast_to(pt, (n, 2)) if pt.ndim == 1 and pt.shape == (2,) else pt, "point")
            if len(pt) != n:
                raise ValueError("point: %d bodies, %d points" % (n, len(pt)))
            push["at_point"], push["px"], push["py"] = 1, pt[:, 0], pt[:, 1]
        return push

    def _push(self, fn, bodies, push, wake):
        b = self._body_ids(bodies)
        push = np.ascontiguousarray(push, BODY_PUSH_DTYPE)
        if push.shape != b.shape:
            raise ValueError("%d bodies, push records of shape %s" % (len(b), push.shape))
        _check(fn(self.p, len(b), b.ctypes.data_as(C.c_void_p), push.ctypes.data_as(C.c_void_p), int(bool(wake))))

    def apply_forces(self, bodies, force, torque=0.0, point=None, wake=True):
        """b2hip_apply_force for each body of `bodies` (ids, each once) in one call on the device: `force` (n, 2) or one pair
        for all, `torque` (n,) or one number, `point` (n, 2) or one pair: the world points the forces act at (None: the
        centres of mass). `force` may also be a BODY_PUSH_DTYPE array (then torque and point are not looked at)."""
        b = self._body_ids(bodies)
        if not (isinstance(force, np.ndarray) and force.dtype == BODY_PUSH_DTYPE):
            force = self._pushes(len(b), force, torque, point, "force")
        self._push(self.L.b2hip_apply_forces, b, force, wake)

    def apply_impulses(self, bodies, impulse, angular=0.0, point=None, wake=True):
        """The linear impulse call (at `point`, or at the centre of mass) and then b2hip_apply_angular_impulse for each body of
        `bodies` (ids, each once) in one call on the device; arguments as apply_forces."""
        b = self._body_ids(bodies)
        if not (isinstance(impulse, np.ndarray) and impulse.dtype == BODY_PUSH_DTYPE):
            impulse = self._pushes(len(b), impulse, angular, point, "impulse")
        self._push(self.L.b2hip_apply_impulses, b, impulse, wake)

    def set_velocities(self, bodies, velocity=None, omega=None):
        """b2hip_set_velocity for each body of `bodies` (ids, each once) in one call on the device: `velocity` (n, 2) or one
        pair, `omega` (n,) or one number; what is None keeps its value."""
        if velocity is None and omega is None:
            raise ValueError("set_velocities: neither a velocity nor an omega")
        b = self._body_ids(bodies)
        n = len(b)
        v3 = np.zeros((n, 3), np.float32)
        if velocity is not None:
            v = np.asarray(velocity, np.float32)
            v = self._pairs(np.broadcast_to(v, (n, 2)) if v.ndim == 1 and v.shape == (2,) else v, "velocity")
            if len(v) != n:
                raise ValueError("velocity: %d bodies, %d vectors" % (n, len(v)))
            v3[:, :2] = v
        if omega is not None:
            o = np.asarray(omega, np.float32)
            if o.ndim > 1 or (o.ndim == 1 and len(o) != n):
                raise ValueError("omega: %d bodies, shape %s" % (n, o.shape))
            v3[:, 2] = o
        mask = (1 if velocity is not None else 0) | (2 if omega is not None else 0)
        _check(self.L.b2hip_set_velocities(self.p, n, b.ctypes.data_as(C.c_void_p), v3.ctypes.data_as(C.c_void_p), mask))

    def body_states_of(self, bodies):
        """The BODY_STATE_DTYPE rows of `bodies` (ids; one may occur again), gathered on the device: body_states()[bodies]
        without the table crossing."""
        b = self._body_ids(bodies)
        out = np.zeros(len(b), BODY_STATE_DTYPE)
        _check(self.L.b2hip_get_body_states_of(self.p, len(b), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- batched teleports and sleep / wake sets on the device (include/b2hip.h, block H: b2hip_set_transforms,
    # b2hip_set_awakes)
    def set_transforms(self, bodies, position=None, angle=None):
        """b2hip_set_transform for each body of `bodies` (ids, each once) in one call on the device: `position` (n, 2) or one
        pair, `angle` (n,) or one number; what is None keeps its value. The bodies keep their velocities and do not wake."""
        if position is None and angle is None:
            raise ValueError("set_transforms: neither a position nor an angle")
        b = self._body_ids(bodies)
        n = len(b)
        pose3 = np.zeros((n, 3), np.float32)
        if position is not None:
            p = np.asarray(position, np.float32)
            p = self._pairs(np.broadcast_to(p, (n, 2)) if p.ndim == 1 and p.shape == (2,) else p, "position")
            if len(p) != n:
                raise ValueError("position: %d bodies, %d vectors" % (n, len(p)))
            pose3[:, :2] = p
        if angle is not None:
            a = np.asarray(angle, np.float32)
            if a.ndim > 1 or (a.ndim == 1 and len(a) != n):
                raise ValueError("angle: %d bodies, shape %s" % (n, a.shape))
            pose3[:, 2] = a
        mask = (1 if position is not None else 0) | (2 if angle is not None else 0)
        _check(self.L.b2hip_set_transforms(self.p, n, b.ctypes.data_as(C.c_void_p), pose3.ctypes.data_as(C.c_void_p), mask))

    def set_awakes(self, bodies, awake=True):
        """b2hip_set_awake for each body of `bodies` (ids, each once) in one call on the device: `awake` (n,) or one flag for
        all. False also zeroes the velocity and the forces of the body."""
        b = self._body_ids(bodies)
        n = len(b)
        flags = np.asarray(awake)
        if flags.ndim > 1 or (flags.ndim == 1 and len(flags) != n):
            raise ValueError("awake: %d bodies, shape %s" % (n, flags.shape))
        flags = np.ascontiguousarray(np.broadcast_to(flags != 0, (n,)), np.uint8)
        _check(self.L.b2hip_set_awakes(self.p, n, b.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p)))

    # ---- batched destruction and activation sets on the device (include/b2hip.h, block I: b2hip_destroy_bodies,
    # b2hip_set_actives)
    def destroy_bodies(self, bodies):
        """b2hip_destroy_body for each body of `bodies` (ids, each once) in one call on the device: the bodies, their fixtures
        and their contacts (ids are never reused). A batch that names a body with a live joint runs the single calls."""
        b = self._body_ids(bodies)
        _check(self.L.b2hip_destroy_bodies(self.p, len(b), b.ctypes.data_as(C.c_void_p)))

    def set_actives(self, bodies, active=True):
        """b2hip_set_active for each body of `bodies` (ids, each once) in one call on the device: `active` (n,) or one flag
        for all. A body that has the requested state already is left alone."""
        b = self._body_ids(bodies)
        n = len(b)
        flags = np.asarray(active)
        if flags.ndim > 1 or (flags.ndim == 1 and len(flags) != n):
            raise ValueError("active: %d bodies, shape %s" % (n, flags.shape))
        flags = np.ascontiguousarray(np.broadcast_to(flags != 0, (n,)), np.uint8)
        _check(self.L.b2hip_set_actives(self.p, n, b.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p)))

    # ---- batched fixture sets on the device (include/b2hip.h, block J: b2hip_fixture_set_filters, b2hip_fixture_set_sensors,
    # b2hip_fixture_set_thicks, b2hip_fixture_set_materials)
    @staticmethod
    def _fixture_ids(fixtures):
        f = np.ascontiguousarray(fixtures, np.int32)
        if f.ndim != 1:
            raise ValueError("fixtures: an (n,) array of fixture ids is expected, got shape %s" % (f.shape,))
        return f

    @staticmethod
    def _per_fixture(value, n, dtype, name):
        """`value` as n entries of `dtype`: (n,) or one for all"""
        v = np.asarray(value)
        if v.ndim > 1 or (v.ndim == 1 and len(v) != n):
            raise ValueError("%s: %d fixtures, shape %s" % (name, n, v.shape))
        return np.broadcast_to(v, (n,)).astype(dtype)

    def fixture_set_filters(self, fixtures, category_bits, mask_bits, group_index=0):
        """b2hip_fixture_set_filter for each fixture of `fixtures` (ids, each once) in one call on the device: the three filter
        words (n,) or one for all. Every named fixture is re-filtered, as by the single call."""
        f = self._fixture_ids(fixtures)
        n = len(f)
        rec = np.zeros(n, FIXTURE_FILTER_DTYPE)
        rec["category_bits"] = self._per_fixture(category_bits, n, np.uint16, "category_bits")
        rec["mask_bits"] = self._per_fixture(mask_bits, n, np.uint16, "mask_bits")
        rec["group_index"] = self._per_fixture(group_index, n, np.int16, "group_index")
        _check(self.L.b2hip_fixture_set_filters(self.p, n, f.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)))

    def _fixture_flags(self, fn, fixtures, flag, name):
        f = self._fixture_ids(fixtures)
        flags = np.ascontiguousarray(self._per_fixture(np.asarray(flag) != 0, len(f), np.uint8, name))
        _check(getattr(self.L, fn)(self.p, len(f), f.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p)))

    def fixture_set_sensors(self, fixtures, flag=True):
        """b2hip_fixture_set_sensor for each fixture of `fixtures` (ids, each once) in one call on the device: `flag` (n,) or one
        for all. The body of a fixture that changes wakes; one that has the requested value already is left alone."""
        self._fixture_flags("b2hip_fixture_set_sensors", fixtures, flag, "flag")

    def fixture_set_thicks(self, fixtures, flag=True):
        """b2hip_fixture_set_thick for each fixture of `fixtures` (ids, each once) in one call on the device: `flag` (n,) or one
        for all."""
        self._fixture_flags("b2hip_fixture_set_thicks", fixtures, flag, "flag")

    def fixture_set_materials(self, fixtures, density=None, friction=None, restitution=None):
        """b2hip_fixture_set_material for each fixture of `fixtures` (ids, each once) in one call on the device: each of the
        three (n,) or one number for all; what is None keeps its value."""
        f = self._fixture_ids(fixtures)
        n = len(f)
        rec = np.zeros(n, FIXTURE_MATERIAL_DTYPE)
        mask = 0
        for bit, name, value in ((MATERIAL_DENSITY, "density", density), (MATERIAL_FRICTION, "friction", friction),
                                 (MATERIAL_RESTITUTION, "restitution", restitution)):
            if value is not None:
                rec[name] = self._per_fixture(value, n, np.float32, name)
                mask |= bit
        if mask == 0:
            raise ValueError("fixture_set_materials: neither a density nor a friction nor a restitution")
        _check(self.L.b2hip_fixture_set_materials(self.p, n, f.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), mask))

    # ---- batched body property sets on the device (include/b2hip.h, block K: b2hip_set_types, b2hip_set_bullets,
    # b2hip_set_fixed_rotations, b2hip_set_sleeping_alloweds, b2hip_set_body_dampings, b2hip_set_mass_datas, b2hip_reset_mass_datas)
    @staticmethod
    def _per_body(value, n, dtype, name):
        """`value` as n entries of `dtype`: (n,) or one for all"""
        v = np.asarray(value)
        if v.ndim > 1 or (v.ndim == 1 and len(v) != n):
            raise ValueError("%s: %d bodies, shape %s" % (name, n, v.shape))
        return np.ascontiguousarray(np.broadcast_to(v, (n,)).astype(dtype))

    def _body_flags(self, fn, bodies, flag, name):
        b = self._body_ids(bodies)
        flags = self._per_body(np.asarray(flag) != 0, len(b), np.uint8, name)
        _check(getattr(self.L, fn)(self.p, len(b), b.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p)))

    def set_types(self, bodies, type):
        """b2hip_set_type for each body of `bodies` (ids, each once) in one call on the device: `type` (n,) or one for all,
        STATIC, KINEMATIC or DYNAMIC. A body that has the requested type already is left alone."""
        b = self._body_ids(bodies)
        t = np.asarray(type)
        if t.ndim <= 1 and t.size and (np.any(t < 0) or np.any(t > 255)):
            raise ValueError("type: a body type is STATIC, KINEMATIC or DYNAMIC")
        types = self._per_body(t, len(b), np.uint8, "type")
        _check(self.L.b2hip_set_types(self.p, len(b), b.ctypes.data_as(C.c_void_p), types.ctypes.data_as(C.c_void_p)))

    def set_bullets(self, bodies, flag=True):
        """b2hip_set_bullet for each body of `bodies` (ids, each once) in one call on the device: `flag` (n,) or one for all."""
        self._body_flags("b2hip_set_bullets", bodies, flag, "flag")

    def set_fixed_rotations(self, bodies, flag=True):
        """b2hip_set_fixed_rotation for each body of `bodies` (ids, each once) in one call on the device: `flag` (n,) or one
        for all. A body that changes stops spinning and gets its mass data again."""
        self._body_flags("b2hip_set_fixed_rotations", bodies, flag, "flag")

    def set_sleeping_alloweds(self, bodies, flag=True):
        """b2hip_set_sleeping_allowed for each body of `bodies` (ids, each once) in one call on the device: `flag` (n,) or one
        for all. False wakes the body."""
        self._body_flags("b2hip_set_sleeping_alloweds", bodies, flag, "flag")

    def set_body_dampings(self, bodies, linear=None, angular=None, gravity_scale=None):
        """b2hip_set_body_damping for each body of `bodies` (ids, each once) in one call on the device: each of the three (n,)
        or one number for all; what is None keeps its value."""
        b = self._body_ids(bodies)
        n = len(b)
        rec = np.zeros(n, BODY_DAMPING_DTYPE)
        mask = 0
        for bit, name, value in ((DAMPING_LINEAR, "linear_damping", linear), (DAMPING_ANGULAR, "angular_damping", angular),
                                 (DAMPING_GRAVITY_SCALE, "gravity_scale", gravity_scale)):
            if value is not None:
                rec[name] = self._per_body(value, n, np.float32, name)
                mask |= bit
        if mask == 0:
            raise ValueError("set_body_dampings: neither a linear nor an angular damping nor a gravity scale")
        _check(self.L.b2hip_set_body_dampings(self.p, n, b.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), mask))

    def set_mass_datas(self, bodies, mass, inertia, local_center):
        """b2hip_set_mass_data for each body of `bodies` (ids, each once) in one call on the device: `mass` and `inertia` (about
        the body's origin) (n,) or one number for all, `local_center` (n, 2) or one pair."""
        b = self._body_ids(bodies)
        n = len(b)
        rec = np.zeros(n, MASS_DATA_DTYPE)
        rec["mass"] = self._per_body(mass, n, np.float32, "mass")
        rec["inertia"] = self._per_body(inertia, n, np.float32, "inertia")
        c = np.asarray(local_center, np.float32)
        c = self._pairs(np.broadcast_to(c, (n, 2)) if c.ndim == 1 and c.shape == (2,) else c, "local_center")
        if len(c) != n:
            raise ValueError("local_center: %d bodies, %d centres" % (n, len(c)))
        rec["local_center"] = c
        _check(self.L.b2hip_set_mass_datas(self.p, n, b.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)))

    def reset_mass_datas(self, bodies):
        """b2hip_set_mass_data(body, NULL) - b2Body::ResetMassData - for each body of `bodies` (ids, each once) in one call."""
        b = self._body_ids(bodies)
        _check(self.L.b2hip_reset_mass_datas(self.p, len(b), b.ctypes.data_as(C.c_void_p)))

    # ---- batched joints on the device (include/b2hip.h, block G: b2hip_joint_set_motors, b2hip_get_joint_states) and the
    # single-joint reads they are defined by
    @property
    def joint_count(self):
        return self.L.b2hip_joint_count(self.p)

    def joint_is_destroyed(self, joint):
        return bool(self.L.b2hip_joint_is_destroyed(self.p, joint))

    def joint_reaction(self, joint, inv_dt=60.0):
        """b2hip_get_joint_reaction: (force x, force y, torque, motor torque / force) of the last step as 4 float32."""
        out = np.zeros(4, np.float32)
        _check(self.L.b2hip_get_joint_reaction(self.p, joint, inv_dt, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def joint_limit_state(self, joint):
        """b2hip_get_joint_limit_state: 0 inactive, 1 at lower, 2 at upper, 3 equal limits."""
        return _check(self.L.b2hip_get_joint_limit_state(self.p, joint))

    @staticmethod
    def _joint_ids(joints):
        j = np.ascontiguousarray(joints, np.int32)
        if j.ndim != 1:
            raise ValueError("joints: an (n,) array of joint ids is expected, got shape %s" % (j.shape,))
        return j

    @staticmethod
    def _joint_motors(n, speed, max_motor, enable):
        """(n JOINT_MOTOR_DTYPE records, mask) of what is given: each of `speed`, `max_motor`, `enable` None (the joint keeps its
        value), one number for all, or (n,)."""
        motors = np.zeros(n, JOINT_MOTOR_DTYPE)
        mask = 0
        for value, field, bit, kind in ((enable, "enable_motor", JOINT_MOTOR_ENABLE, bool), (speed, "motor_speed", JOINT_MOTOR_SPEED, np.float32),
                                        (max_motor, "max_motor", JOINT_MOTOR_MAX, np.float32)):
            if value is None:
                continue
            v = np.asarray(value, kind)
            if v.ndim > 1 or (v.ndim == 1 and len(v) != n):
                raise ValueError("%s: %d joints, shape %s" % (field, n, v.shape))
            motors[field] = v
            mask |= bit
        if mask == 0:
            raise ValueError("joint_set_motors: none of speed, max_motor and enable is given")
        return motors, mask

    def joint_set_motors(self, joints, speed=None, max_motor=None, enable=None, mask=None):
        """b2hip_joint_set_motor for each joint of `joints` (revolute, prismatic or wheel; ids, each once) in one call on the
        device: `speed`, `max_motor` and `enable` are one value for all or (n,); what is None keeps its value. `speed` may also
        be a JOINT_MOTOR_DTYPE array, taken as it is with an explicit mask= (1: enable_motor, 2: motor_speed, 4: max_motor)."""
        j = self._joint_ids(joints)
        if isinstance(speed, np.ndarray) and speed.dtype == JOINT_MOTOR_DTYPE:
            if mask is None or max_motor is not None or enable is not None:
                raise ValueError("joint_set_motors: a JOINT_MOTOR_DTYPE array goes with mask= and nothing else")
            motors = np.ascontiguousarray(speed)
            if motors.shape != j.shape:
                raise ValueError("%d joints, motor records of shape %s" % (len(j), motors.shape))
        else:
            if mask is not None:
                raise ValueError("joint_set_motors: mask= goes with a JOINT_MOTOR_DTYPE array only")
            motors, mask = self._joint_motors(len(j), speed, max_motor, enable)
        _check(self.L.b2hip_joint_set_motors(self.p, len(j), j.ctypes.data_as(C.c_void_p), motors.ctypes.data_as(C.c_void_p), int(mask)))

    def joint_states(self, joints, inv_dt=60.0):
        """One JOINT_STATE_DTYPE record per joint of `joints` (ids; one may occur again), computed on the device: type (-1:
        destroyed), limit state, the joint's coordinate(s) and speed(s), and the reaction force, torque and motor share of the
        last step scaled by inv_dt."""
        j = self._joint_ids(joints)
        out = np.zeros(len(j), JOINT_STATE_DTYPE)
        _check(self.L.b2hip_get_joint_states(self.p, len(j), j.ctypes.data_as(C.c_void_p), inv_dt, out.ctypes.data_as(C.c_void_p)))
        return out

    def solver_timing(self):
        ms, by, ct, b = C.c_float(), C.c_double(), C.c_int(), C.c_int()
        _check(self.L.b2hip_get_solver_timing(self.p, C.byref(ms), C.byref(by), C.byref(ct), C.byref(b)))
        return ms.value, by.value, ct.value, b.value
