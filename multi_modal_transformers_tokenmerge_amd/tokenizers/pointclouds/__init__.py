from .depth import depth_to_point_cloud  # noqa: F401
