"""Primary rays for cameras the scene's own pinhole is not: acn_render_rays (include/actinon_hip.h) renders any [n, 6] array
of rays (origin, direction), and these functions make such arrays."""
import numpy as np


def _unit(v):
    v = np.asarray(v, dtype=np.float64).reshape(3)
    return v / np.sqrt(v @ v)


def panorama_rays(origin, view, top, width, height):
    """Equirectangular 360-degree panorama seen from `origin`: float64 [height * width, 6] rays (origin, unit direction)
    through the pixel centres, row-major.  Longitude 0 looks along `view` and lies at the centre of the image; it grows to
    the right, towards view x top (the right of the scene's pinhole camera).  Latitude rises toward `top`: +90 degrees at
    the top edge of the image, -90 at the bottom.  Only an odd width has a centre column at longitude 0 and only an odd
    height an equator row (an even size puts the two middle pixels half a pixel to either side), so the ray of the middle
    pixel looks exactly along `view` when both are odd."""
    fwd = _unit(view)
    t = np.asarray(top, dtype=np.float64).reshape(3)
    t = t - (t @ fwd) * fwd
    if not np.sqrt(t @ t) > 1e-12:
        raise ValueError("panorama_rays: top is parallel to view")
    up = _unit(t)
    right = np.cross(fwd, up)
    lon = ((np.arange(width) + 0.5) / width - 0.5) * (2.0 * np.pi)
    lat = (0.5 - (np.arange(height) + 0.5) / height) * np.pi
    horizontal = np.cos(lon)[:, None] * fwd + np.sin(lon)[:, None] * right                  # [width, 3]
    d = np.cos(lat)[:, None, None] * horizontal[None] + np.sin(lat)[:, None, None] * up     # [height, width, 3]
    d = d.reshape(-1, 3)
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    rays = np.empty((width * height, 6), dtype=np.float64)
    rays[:, :3] = np.asarray(origin, dtype=np.float64).reshape(3)
    rays[:, 3:] = d
    return rays


def orbit_camera(params, degrees, target_distance=None):
    """The scene's pinhole camera moved on a circle around its view target, for Handle.set_params: `params` is an abi.Params (or
    anything with camera_position, camera_view_direction, camera_top_direction), the target the point target_distance along the view
    direction (None: the length of camera_view_direction, which is how the shipped scenes state what they look at), the axis the top
    direction through the target.  Returns dict( camera_position=..., camera_view_direction=... ); the top direction and the length of
    the view direction stay."""
    pos = np.array([params.camera_position[i] for i in range(3)], dtype=np.float64)
    view = np.array([params.camera_view_direction[i] for i in range(3)], dtype=np.float64)
    axis = _unit([params.camera_top_direction[i] for i in range(3)])
    target = pos + (view if target_distance is None else _unit(view) * float(target_distance))
    a = np.deg2rad(float(degrees))

    def turn(v):                                   # Rodrigues' rotation about `axis`
        return v * np.cos(a) + np.cross(axis, v) * np.sin(a) + axis * (axis @ v) * (1.0 - np.cos(a))

    return dict(camera_position=tuple(float(x) for x in target + turn(pos - target)),
                camera_view_direction=tuple(float(x) for x in turn(view)))
