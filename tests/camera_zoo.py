"""Cameras away from samples.SAMPLES, and the resolver the reference modules
use to take either kind (not a test).

samples.SAMPLES holds one camera per model, and those sit in one corner of
the parameter space: RadTan with k3 = 0, DS / UCM / EUCM all with alpha > 0.5,
one FOV w.  Each camera here is named for the branch or regime it is there
for; tests/test_camera_zoo_ref.py pins the CPU oracle to 50-digit mpmath at
every one of them before the oracle judges a kernel there.

camera_of(key): key is a model id (the sample camera, exactly
samples.SAMPLES[key]) or a zoo name.
"""
from apex_camera_models import samples

_KB_SAMPLE = samples.SAMPLES[2][0][:4]

# (name, model, params, (width, height), note)
ZOO = (
    ("pinhole_aniso", 0, [800.0, 400.0, 100.5, 400.25], (640, 512),
     "fx = 2 fy, principal point far off the centre"),
    ("pinhole_short", 0, [150.0, 152.0, 330.0, 236.0], (640, 480),
     "short focal length: steep rays, most of the wide point set lands inside the image"),
    ("radtan_k3_tangential", 1,
     [461.629, 460.152, 362.68, 246.049, -0.28, 0.074, 0.0012, -0.0021, -0.011], (752, 480),
     "k3 != 0 and tangential terms of either sign, 100 x the sample's p2"),
    ("radtan_barrel_pos", 1, [600.0, 598.0, 640.0, 360.0, 0.12, -0.03, -0.004, 0.003, 0.006],
     (1280, 720), "k1 > 0, k3 > 0"),
    ("kb_strong", 2, list(_KB_SAMPLE) + [0.5, -0.3, 0.1, -0.02], (512, 512),
     "strong distortion: theta_d is not monotone over the image"),
    ("kb_negative", 2, [300.0, 310.0, 320.0, 240.0, -0.2, 0.15, -0.05, 0.004], (640, 480),
     "k1 < 0, alternating signs"),
    ("ds_alpha_lt_half", 3, [350.0, 351.0, 366.0, 249.0, 0.35, 0.2], (752, 480),
     "alpha <= 0.5: w1 = alpha / (1 - alpha), no unprojection condition"),
    ("ds_alpha_half", 3, [350.0, 351.0, 366.0, 249.0, 0.5, -0.1], (752, 480),
     "alpha = 0.5 exactly: 1 / (2 alpha - 1) is 1 / 0"),
    ("ds_alpha_one", 3, [350.0, 351.0, 366.0, 249.0, 1.0, 0.6], (752, 480),
     "alpha = 1: w1 = 0"),
    ("ds_xi_pos", 3, [350.0, 351.0, 366.0, 249.0, 0.72, 0.9], (752, 480),
     "xi > 0, close to its limit 1"),
    ("ucm_alpha_lt_half", 4, [400.0, 402.0, 376.0, 240.0, 0.3], (752, 480),
     "alpha <= 0.5: w = alpha / (1 - alpha), no unprojection condition"),
    ("ucm_alpha_half", 4, [400.0, 402.0, 376.0, 240.0, 0.5], (752, 480),
     "alpha = 0.5 exactly"),
    ("ucm_alpha_mid", 4, [400.0, 402.0, 376.0, 240.0, 0.62], (752, 480),
     "0.5 < alpha < 1 (the sample has alpha > 1)"),
    ("eucm_alpha_lt_half", 5, [400.0, 402.0, 376.0, 240.0, 0.3, 1.2], (752, 480),
     "alpha <= 0.5: both conditions are constant true"),
    ("eucm_alpha_half", 5, [400.0, 402.0, 376.0, 240.0, 0.5, 2.0], (752, 480),
     "alpha = 0.5 exactly, beta = 2"),
    ("eucm_alpha_mid", 5, [900.0, 902.0, 376.0, 240.0, 0.65, 1.1], (752, 480),
     "0.5 < alpha < 1; long focal length so that r^2 <= (1 / beta)(2 alpha - 1) holds "
     "over the whole image"),
    ("fov_narrow", 6, [379.045, 379.008, 376.0, 240.0, 0.2], (752, 480),
     "small w: rd w stays far below 1"),
    ("fov_mid", 6, [379.045, 379.008, 376.0, 240.0, 1.6], (752, 480),
     "rd w between pi / 2 and 2 in the corners: cos(rd w) < 0, sin / cos still polynomial"),
    ("fov_max", 6, [180.0, 181.0, 376.0, 240.0, 2.9], (752, 480),
     "rd w up to ~5: the model folds over, the library sin / cos fallback; per-point "
     "kernels only"),
)

NAMES = tuple(z[0] for z in ZOO)
_BY_NAME = {z[0]: z for z in ZOO}

# one or two cameras per model for the solver sums (never fov_max)
SOLVER_SUBSET = ("pinhole_aniso", "radtan_k3_tangential", "kb_negative", "ds_alpha_lt_half",
                 "ds_xi_pos", "ucm_alpha_lt_half", "eucm_alpha_half", "fov_mid")


def camera_of(key):
    """(model id, params, (width, height)) of a model id's sample camera or of
    a zoo name."""
    if isinstance(key, str):
        _, model, params, res, _ = _BY_NAME[key]
        return model, params, res
    params, res = samples.SAMPLES[key]
    return key, params, res


def label(key):
    """What a test prints for the camera: the zoo name or the model's name."""
    return key if isinstance(key, str) else samples.MODEL_NAMES[key]


def device_model(key, params=None):
    """The package's camera object for `key` (optionally with other parameters)."""
    from apex_camera_models import Resolution
    from apex_camera_models.camera import MODEL_CLASSES
    model, p, (w, h) = camera_of(key)
    return MODEL_CLASSES[samples.MODEL_NAMES[model]]._from_params(
        list(p if params is None else params), Resolution(w, h))
