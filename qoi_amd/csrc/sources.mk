# The translation units of libqoi_mi355x.so: every *.hip of this directory, one object each (no .hip file includes another; tests/test_abi.py
# holds both).  Included by this directory's Makefile (all three flavours) and by tests/fuzz/Makefile (the sanitizer build).
# The two that take longest to compile stand first: a parallel make begins with them.
SRCS := qoi_decode.hip qoi_encode.hip qoi_synth.hip \
        qoi_pack.hip qoi_inspect.hip qoi_compare.hip qoi_thumb.hip qoi_crop.hip qoi_resize.hip qoi_warp.hip qoi_warp_cubic.hip qoi_warp_border.hip qoi_warp_super.hip qoi_warp_vote.hip qoi_warp_proj.hip qoi_tensor.hip qoi_cubic.hip qoi_lanczos.hip qoi_nearest.hip qoi_mode.hip qoi_stats.hip qoi_seek.hip qoi_tile.hip qoi_ingest.hip qoi_label.hip \
        qoi_host.hip qoi_host_encode.hip qoi_host_decode.hip qoi_host_pack.hip qoi_host_staged.hip qoi_host_tensor.hip qoi_host_seek.hip
