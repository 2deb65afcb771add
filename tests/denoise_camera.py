"""The camera offset shared by the denoiser's CPU and GPU feature tests (no
test of its own).  The box scenes' own camera sits on the room's axis: at
64x48 pixel centres then fall exactly on the seams between two walls, where
fp32 and double break the tie differently
(tests/test_denoise_host.py::test_on_axis_box_camera_puts_pixel_centres_on_wall_seams);
a camera a little off the axis has no such pixel
(test_first_hit_reference_stays_inside_its_cap)."""
OFF_AXIS = (0.013, 0.021, 0.0)
