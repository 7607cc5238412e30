"""The camera models the ``Undistorted`` task reads (``plant3dvision/camera.py``), as far as the lens correction
needs them: the three COLMAP models ``SIMPLE_RADIAL`` (f, cx, cy, k), ``RADIAL`` (f, cx, cy, k1, k2) and ``OPENCV``
(fx, fy, cx, cy, k1, k2, p1, p2), from a parameter list to named parameters to the camera matrix and distortion vector
``cv2.undistort`` takes.  The arrays are **float32**, as the reference's are (camera.py:104-128): the lens correction
widens them to float64, so the values it computes with are the float32-rounded ones.
"""
import numpy as np

VALID_MODELS = ("OPENCV", "RADIAL", "SIMPLE_RADIAL")

#: parameter names of a model, in the order of its COLMAP parameter list
MODEL_PARAMS = {
    "SIMPLE_RADIAL": ("f", "cx", "cy", "k"),
    "RADIAL": ("f", "cx", "cy", "k1", "k2"),
    "OPENCV": ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"),
}


def camera_kwargs_from_params_list(model, params):
    """Named parameters of a COLMAP parameter list: ``{'model': ..., name: value, ...}`` in the model's order
    (``get_camera_kwargs_from_params_list``, camera.py:222-304).  An ``OPENCV`` list with ``fx == fy`` and
    ``p1 == p2 == 0`` is reported as the simpler model it is: ``SIMPLE_RADIAL`` if also ``k1 == k2`` (the reference's
    own test, :281), else ``RADIAL``.  An unknown model gives ``{}``."""
    model = model.upper()
    if model not in MODEL_PARAMS:
        return {}
    named = dict(zip(MODEL_PARAMS[model], params))
    if model == "OPENCV" and named["fx"] == named["fy"] and named["p1"] == named["p2"] == 0.:
        if named["k1"] == named["k2"]:
            model, named = "SIMPLE_RADIAL", {"f": named["fx"], "cx": named["cx"], "cy": named["cy"], "k": named["k1"]}
        else:
            model, named = "RADIAL", {"f": named["fx"], "cx": named["cx"], "cy": named["cy"], "k1": named["k1"],
                                      "k2": named["k2"]}
    return {"model": model, **named}


def camera_arrays_from_params(model, **kwargs):
    """``(camera matrix float32 [3, 3], distortion vector float32 [4] = k1, k2, p1, p2)`` of a model's named
    parameters (``get_camera_arrays_from_params``, camera.py:104-138); further keywords are ignored, an unknown model
    gives ``None`` as the reference does."""
    model = model.lower()
    if model == "opencv":
        fx, fy, d = kwargs["fx"], kwargs["fy"], [kwargs["k1"], kwargs["k2"], kwargs["p1"], kwargs["p2"]]
    elif model == "radial":
        fx = fy = kwargs["f"]
        d = [kwargs["k1"], kwargs["k2"], 0., 0.]
    elif model == "simple_radial":
        fx = fy = kwargs["f"]
        d = [kwargs["k"], 0., 0., 0.]
    else:
        return None
    camera = np.array([[fx, 0, kwargs["cx"]], [0, fy, kwargs["cy"]], [0, 0, 1]], dtype="float32")
    return camera, np.array(d, dtype="float32")


def camera_kwargs_from_images_metadata(file):
    """The named camera parameters in a picture file's ``colmap_camera`` metadata, ``None`` if it has none
    (``get_camera_kwargs_from_images_metadata``, camera.py:307-334)."""
    colmap_camera = file.get_metadata("colmap_camera")
    if colmap_camera is None:
        return None
    camera_model = colmap_camera["camera_model"]
    return camera_kwargs_from_params_list(camera_model["model"], camera_model["params"])
