"""The frames of tests/test_gpu_arith_paths.py, shared with the host tier (tests/test_arith_paths_frames_cpu.py): plain data, no device."""

# part a: the frame scenes of tests/test_gpu_mesh_walks.py for the mesh cases of tests/arithcases.py (not the NaN / tie scenes)
MESH_FRAMES = ["chain", "chain_deep", "chain_and_hull", "twins", "geoms32", "boundary", "boundary23_alone"]

# part b
# name: (scene file or None = the 70-material scene, resolution, depth, options, switch set to "1" or None, what the forced specialised
#        kernel must refuse with (a regular expression) or None = it must be accepted or is not asked)
PATHS = {
    "general_kernel": ("cornellObj.txt", (96, 64), 6, {}, "PTX_DEBUG_NO_FAST", None),
    "specialised_kernel": ("cornellObj.txt", (96, 64), 6, {}, "PTX_DEBUG_FORCE_FAST", None),
    "full_last_bounce": ("cornellObj.txt", (96, 64), 6, {}, "PTX_DEBUG_NO_LAST", None),
    "unsorted": ("cornellObj.txt", (96, 64), 6, dict(sort_by_material=0), None, "sort_by_material"),
    "bins70_geoms40": (None, (120, 90), 6, {}, None, None),
    "textured_mesh_unsplit": ("cornellSpaceship.txt", (96, 54), 8, dict(no_mesh_split=1), None, "split mesh|textured|BVH"),
    "textured_mesh_split": ("cornellSpaceship.txt", (96, 54), 8, {}, None, None),
    "depth_of_field": ("cornellGlass.txt", (96, 64), 8, dict(depth_of_field=1), None, "depth of field"),
    # (128 x 96, not a square frame: tests/test_arith_paths_frames_cpu.py -- on square frames of this scene the oracle's own two builds
    # differ on 8.5 % of the pixels at 1 spp, above the bound the statistical part asserts)
    "first_bounce_cache": ("cornell.txt", (128, 96), 8, dict(antialiasing=0), None, "cache-filling"),
    "apps_variant": ("cornellObj.txt", (96, 64), 6, dict(apps_variant=1), None, None),
    "no_cull": ("cornellObj.txt", (96, 64), 6, dict(no_cull=1), None, None),
    "row_tile": ("cornellObj.txt", (160, 96), 6, dict(tile_rows=8, tile_rank=1, tile_world=2), None, None),
}
