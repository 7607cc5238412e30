"""The ``Masks`` task logic of the reference (``plant3dvision/tasks/proc2d.py:146-249``) around the device mask
producer (``proc2d.masks_from_images``).

As with ``tasks/cl.py::voxels_run``, the task's *logic* -- read every picture, filter, threshold, dilate, the
output metadata -- is a plain function, ``masks_run``, without luigi / plantdb.  The reference runs ``Masks.f`` file
by file; here pictures of equal size go to the device as one batch (every picture still has its own range).
INTEGRATION.md has the lines a maintainer of the reference puts into ``Masks.run``.

``undistorted_run`` is the same for the task in front of it, ``Undistorted`` (tasks/proc2d.py:26-143), around
``proc2d.undistort``: pictures of one size and one camera make one batch.
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)

#: parameter defaults of the reference task (tasks/proc2d.py:207-211)
MASKS_DEFAULTS = dict(type="linear", parameters=[0, 1, 0], threshold=0.3, dilation=0)


def undistorted_run(image_files, camera_model_src="Colmap", upstream_task="ImagesFilesetExists", undistort_fn=None):
    """The ``Undistorted.run`` / ``.f`` loop without luigi / plantdb (tasks/proc2d.py:90-143).

    image_files : list of file-like objects (``.id``, ``.get_metadata``; pixels via ``cl.read_image``), uint8 RGB
        pictures with their camera in the ``colmap_camera`` metadata (whatever ``camera_model_src`` put it there:
        :106-113 happen before this loop).
    undistort_fn : ``proc2d.undistort`` by default; an argument only, the CPU tests pass a function of theirs.

    The reference corrects file by file; here the files of one picture shape and one camera go to the device as one
    batch.  A file without ``colmap_camera`` is logged as an error and left out (:141-143).  Returns
    ``[(id, picture, metadata), ...]`` in input order: ``metadata`` is the input file's with what ``f`` sets (:138)
    over it (:116-118).
    """
    if undistort_fn is None:  # the product: the HIP kernels
        from ..proc2d import undistort as undistort_fn
    from ..camera import camera_arrays_from_params, camera_kwargs_from_images_metadata
    from ..cl import read_image
    logger.info(f"Processing a list of {len(image_files)} image files...")
    groups, cameras = {}, {}  # files of one shape and one camera make one batch, in input order
    pictures = [None] * len(image_files)
    for q, fi in enumerate(image_files):
        cam_kwargs = camera_kwargs_from_images_metadata(fi)
        if cam_kwargs is None:
            logger.error(f"Could not find a camera model in '{getattr(fi, 'filename', fi.id)}' metadata!")
            continue
        pictures[q] = np.asarray(read_image(fi))
        camera_mtx, distortion_vect = camera_arrays_from_params(**cam_kwargs)
        key = (pictures[q].shape, camera_mtx.tobytes(), distortion_vect.tobytes())
        groups.setdefault(key, []).append(q)
        cameras[key] = (camera_mtx, distortion_vect)
    for key, members in groups.items():
        out = undistort_fn(np.stack([pictures[q] for q in members]), *cameras[key])
        for k, q in enumerate(members):
            pictures[q] = out[k]
    md = {"upstream_task": str(upstream_task), "Camera model source": str(camera_model_src)}
    return [(fi.id, pictures[q], {**_file_metadata(fi), **md}) for q, fi in enumerate(image_files) if pictures[q] is not None]


def _file_metadata(fi):
    md = fi.get_metadata()
    return dict(md) if md else {}


def _plain_query(query):
    """The ``query`` dictionary as the reference stores it in the metadata (its ``jsonify``, utils.py:38-64):
    NumPy arrays and numbers as plain Python ones, an empty sequence as ``'None'``."""
    out = {}
    for key, val in dict(query).items():
        if isinstance(val, np.ndarray):
            val = val.tolist()
        if hasattr(val, "__iter__"):
            if len(val) == 0:
                out[key] = "None"
            elif isinstance(val, (list, tuple)) and isinstance(val[0], (float, np.floating)):
                out[key] = [float(x) for x in val]
            elif isinstance(val, (list, tuple)) and isinstance(val[0], np.integer):
                out[key] = [int(x) for x in val]
            else:
                out[key] = val
        elif isinstance(val, (float, np.floating)):
            out[key] = float(val)
        elif isinstance(val, np.integer):
            out[key] = int(val)
        else:
            out[key] = val
    return out


def masks_metadata(type, parameters, threshold, dilation, query=None, upstream_task="Undistorted"):
    """The metadata ``Masks.f`` sets on every mask file (tasks/proc2d.py:242-248)."""
    md = {"upstream_task": str(upstream_task), "filter": str(type), "threshold": threshold, "dilation": dilation}
    if type == "linear":
        md["linear_coeff"] = list(parameters)
    if query is not None and dict(query) != {}:
        md["query"] = _plain_query(query)
    return {"Masks": md}


def masks_run(image_files, type="linear", parameters=(0, 1, 0), threshold=0.3, dilation=0, query=None,
              upstream_task="Undistorted", masks_fn=None):
    """The ``Masks.f`` loop without luigi / plantdb (tasks/proc2d.py:224-249).

    image_files : list of file-like objects (``.id``; pixels via ``cl.read_image``), uint8 RGB pictures.
    masks_fn : ``masks_from_images`` by default; an argument only, the CPU tests pass a function of theirs.

    Returns ``[(id, mask, metadata), ...]`` in input order: ``mask`` the uint8 0 / 255 picture the reference
    writes (:237-240), ``metadata`` what it sets on the file (:242-248).
    """
    if type not in ("linear", "excess_green"):
        raise Exception(f"Unknown masking type '{type}'!")  # tasks/proc2d.py:222
    if masks_fn is None:  # the product: the HIP kernels
        from ..proc2d import masks_from_images as masks_fn
    from ..cl import read_image
    logger.info(f"Processing a list of {len(image_files)} image files...")
    pictures = [np.asarray(read_image(fi)) for fi in image_files]
    groups = {}  # pictures of one size make one batch, in input order
    for q, img in enumerate(pictures):
        groups.setdefault(img.shape, []).append(q)
    masks = [None] * len(pictures)
    for shape, members in groups.items():
        batch = np.stack([pictures[q] for q in members])
        out = masks_fn(batch, type=type, parameters=list(parameters), threshold=threshold, dilation=dilation)
        for k, q in enumerate(members):
            masks[q] = out[k]
    md = masks_metadata(type, parameters, threshold, dilation, query, upstream_task)
    return [(fi.id, masks[q], {"Masks": dict(md["Masks"])}) for q, fi in enumerate(image_files)]
