"""Inventory of the launch-time kernel choices of ``fpsg_amd/csrc/*.hip`` -- plain data, pinned by
``tests/test_dispatch_cpu.py``.

A row is one place where an ``extern "C"`` entry chooses, from its arguments at launch time, which kernel or which
template instantiation it launches: a size range, an alignment, a null pointer, an explicit variant number, an occupancy
heuristic, a byte threshold, a switch read from the environment.  Launch geometry alone (grid, threads, dynamic LDS) is
not a row, nor is a stage that an entry appends when an optional output is asked for.  Every row names

  ``entry``    the C entry (two or three where they share the dispatch),
  ``file``     the source file under ``fpsg_amd/csrc``,
  ``kernel``   the instantiation as its demangled name begins after the namespaces,
  ``lines``    the dispatch line as it stands in the source (first), then the lines that define its condition; each is
               one literal, however long, so that it can be searched for,
  ``when``     the condition in words,
  ``cond``     the condition as a Python expression over a case's shape, where it is arithmetic (else ``None``),
  ``cases``    ``(test id, shape)``: GPU tests that reach the instantiation AND compare its result with a reference (an
               oracle restatement, float64, the library, or another kernel that is itself pinned); ``shape`` holds the
               names ``cond`` reads, or is ``None``.

A row with no case fails ``test_dispatch_cpu.py`` unless it carries ``uncovered``: the technical reason why no test of
the suite can reach it (no argument of any entry selects it).  The streaming / non-temporal forms behind the 300 MiB
threshold, ``NT = true``, are reached at small shapes through the second build of the library in which the threshold is
compiled to 0 (fpsg_amd/csrc/Makefile, tests/test_streaming_forms_gpu.py).  ``FILES_WITHOUT_A_CHOICE`` lists the
sources whose entries each launch one fixed sequence of kernels.  ``profiles/dispatch/kernels.txt`` holds the kernel
names of ``rocprofv3 --kernel-trace --stats`` runs of exactly the cases named here (profiles/dispatch/notes.md).
"""

ROWS = [
    # ---- fps.hip -------------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<64, 1>',
        "lines": [
            'if (N <= 64) fps_launch<64, 1>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": 'N <= 64',
        "cond": 'N <= 64',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-2-2]', {'N': 2}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-2-2]', {'N': 2}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[tanh-3-63-63]', {'N': 63}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[tanh-3-63-63]', {'N': 63}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-64-64]', {'N': 64}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-64-64]', {'N': 64}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[lattice-64]', {'N': 64}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[lattice-64]', {'N': 64}),
        ],
    },
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<64, 4>',
        "lines": [
            'else if (N <= 256) fps_launch<64, 4>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": '64 < N <= 256',
        "cond": '64 < N <= 256',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-65-64]', {'N': 65}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-65-64]', {'N': 65}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[tanh-64-100-100]', {'N': 100}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[tanh-64-100-100]', {'N': 100}),
        ],
    },
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<256, 4>',
        "lines": [
            'else if (N <= 1024) fps_launch<256, 4>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": '256 < N <= 1024',
        "cond": '256 < N <= 1024',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-257-64]', {'N': 257}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-257-64]', {'N': 257}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-4-777-333]', {'N': 777}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-4-777-333]', {'N': 777}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[repeated]', {'N': 512}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[repeated]', {'N': 512}),
        ],
    },
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<512, 4>',
        "lines": [
            'else if (N <= 2048) fps_launch<512, 4>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": '1024 < N <= 2048',
        "cond": '1024 < N <= 2048',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-1025-64]', {'N': 1025}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-1025-64]', {'N': 1025}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-37-2048-512]', {'N': 2048}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-37-2048-512]', {'N': 2048}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[lattice]', {'N': 2048}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[lattice]', {'N': 2048}),
        ],
    },
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<1024, 4>',
        "lines": [
            'else if (N <= 4096) fps_launch<1024, 4>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": '2048 < N <= 4096',
        "cond": '2048 < N <= 4096',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-2049-64]', {'N': 2049}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-2049-64]', {'N': 2049}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[tanh-3-4096-64]', {'N': 4096}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[tanh-3-4096-64]', {'N': 4096}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[lattice-4096]', {'N': 4096}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[lattice-4096]', {'N': 4096}),
        ],
    },
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<1024, 8>',
        "lines": [
            'else if (N <= 8192) fps_launch<1024, 8>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": '4096 < N <= 8192',
        "cond": '4096 < N <= 8192',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-4097-32]', {'N': 4097}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-4097-32]', {'N': 4097}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[tanh-3-8192-32]', {'N': 8192}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[tanh-3-8192-32]', {'N': 8192}),
        ],
    },
    {
        "entry": 'fpsg_fps', "file": 'fps.hip',
        "kernel": 'fps_kernel<1024, 16>',
        "lines": [
            'else fps_launch<1024, 16>(xyz, B, N, n, start, idx, min_dist, st);',
        ],
        "when": 'N > 8192',
        "cond": 'N > 8192',
        "cases": [
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-3-8193-32]', {'N': 8193}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-3-8193-32]', {'N': 8193}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[ball-5-15000-2048]', {'N': 15000}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[ball-5-15000-2048]', {'N': 15000}),
            ('tests/test_fps_gpu.py::test_every_checked_round_is_the_argmax_of_k1s_distances[tanh-3-16384-64]', {'N': 16384}),
            ('tests/test_fps_gpu.py::test_every_pick_is_the_float64_farthest_point_up_to_fp32_rounding[tanh-3-16384-64]', {'N': 16384}),
        ],
    },
    # ---- sinkhorn.hip --------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_softmin', "file": 'sinkhorn.hip',
        "kernel": 'softmin_kernel<2>',
        "lines": [
            'if (step_owners_per_lane((long)((N + 127) / 128) * B) == 2)',
            'constexpr int kCUs = 256;',
            'inline int step_owners_per_lane(long workgroups_at_two) { return workgroups_at_two >= 4L * kCUs ? 2 : 1; }',
        ],
        "when": 'ceil(N / 128) * B >= 1024',
        "cond": '-(-N // 128) * B >= 4 * 256',
        "cases": [
            ('tests/test_emd_gpu.py::test_softmin_vs_oracle[1024-70-33-0.05]', {'B': 1024, 'N': 70, 'M': 33}),
            ('tests/test_emd_gpu.py::test_softmin_two_owners_per_lane_equals_one_bit_for_bit[1024-70-33-0.05]', {'B': 1024, 'N': 70, 'M': 33}),
            ('tests/test_emd_gpu.py::test_softmin_vs_oracle[1024-128-129-0.0025]', {'B': 1024, 'N': 128, 'M': 129}),
            ('tests/test_emd_gpu.py::test_softmin_two_owners_per_lane_equals_one_bit_for_bit[1024-128-129-0.0025]', {'B': 1024, 'N': 128, 'M': 129}),
            ('tests/test_emd_gpu.py::test_softmin_vs_oracle[512-129-64-0.5]', {'B': 512, 'N': 129, 'M': 64}),
            ('tests/test_emd_gpu.py::test_softmin_two_owners_per_lane_equals_one_bit_for_bit[512-129-64-0.5]', {'B': 512, 'N': 129, 'M': 64}),
        ],
    },
    {
        "entry": 'fpsg_softmin', "file": 'sinkhorn.hip',
        "kernel": 'softmin_kernel<1>',
        "lines": [
            'hipLaunchKernelGGL((softmin_kernel<1>), dim3((N + 63) / 64, B), dim3(kSmThreads), 0, static_cast<hipStream_t>(stream), x, y, h,',
            'constexpr int kCUs = 256;',
            'inline int step_owners_per_lane(long workgroups_at_two) { return workgroups_at_two >= 4L * kCUs ? 2 : 1; }',
        ],
        "when": 'ceil(N / 128) * B < 1024',
        "cond": 'not (-(-N // 128) * B >= 4 * 256)',
        "cases": [
            ('tests/test_emd_gpu.py::test_softmin_vs_oracle[2-300-500-0.5]', {'B': 2, 'N': 300, 'M': 500}),
            ('tests/test_emd_gpu.py::test_softmin_vs_oracle[1-2500-2100-0.02]', {'B': 1, 'N': 2500, 'M': 2100}),
            ('tests/test_emd_gpu.py::test_softmin_vs_oracle[2-1-7-0.01]', {'B': 2, 'N': 1, 'M': 7}),
        ],
    },
    {
        "entry": 'fpsg_sinkhorn_divergence', "file": 'sinkhorn.hip',
        "kernel": 'sinkhorn_step_kernel<2>',
        "lines": [
            'hipLaunchKernelGGL((sinkhorn_step_kernel<2>), grid, dim3(kSmThreads), 0, s, a);',
            'const int R = step_owners_per_lane((long)((nmax + 127) / 128) * 4 * B);',
            'constexpr int kCUs = 256;',
            'inline int step_owners_per_lane(long workgroups_at_two) { return workgroups_at_two >= 4L * kCUs ? 2 : 1; }',
        ],
        "when": 'ceil(max(N, M) / 128) * 4 * B >= 1024',
        "cond": '-(-max(N, M) // 128) * 4 * B >= 4 * 256',
        "cases": [
            ('tests/test_emd_gpu.py::test_fused_sinkhorn_loop_equals_unfused[256-100-37]', {'B': 256, 'N': 100, 'M': 37}),
            ('tests/test_emd_gpu.py::test_two_owner_sinkhorn_loop_vs_oracle_and_the_one_owner_form[256-100-37]', {'B': 256, 'N': 100, 'M': 37}),
            ('tests/test_emd_gpu.py::test_fused_sinkhorn_loop_equals_unfused[256-70-129]', {'B': 256, 'N': 70, 'M': 129}),
            ('tests/test_emd_gpu.py::test_two_owner_sinkhorn_loop_vs_oracle_and_the_one_owner_form[256-70-129]', {'B': 256, 'N': 70, 'M': 129}),
            ('tests/test_emd_gpu.py::test_fused_sinkhorn_loop_equals_unfused[300-1-9]', {'B': 300, 'N': 1, 'M': 9}),
            ('tests/test_emd_gpu.py::test_two_owner_sinkhorn_loop_vs_oracle_and_the_one_owner_form[300-1-9]', {'B': 300, 'N': 1, 'M': 9}),
        ],
    },
    {
        "entry": 'fpsg_sinkhorn_divergence', "file": 'sinkhorn.hip',
        "kernel": 'sinkhorn_step_kernel<1>',
        "lines": [
            'hipLaunchKernelGGL((sinkhorn_step_kernel<1>), grid, dim3(kSmThreads), 0, s, a);',
            'const int R = step_owners_per_lane((long)((nmax + 127) / 128) * 4 * B);',
            'constexpr int kCUs = 256;',
            'inline int step_owners_per_lane(long workgroups_at_two) { return workgroups_at_two >= 4L * kCUs ? 2 : 1; }',
        ],
        "when": 'ceil(max(N, M) / 128) * 4 * B < 1024',
        "cond": 'not (-(-max(N, M) // 128) * 4 * B >= 4 * 256)',
        "cases": [
            ('tests/test_emd_gpu.py::test_sinkhorn_divergence', {'B': 3, 'N': 512, 'M': 512}),
            ('tests/test_emd_gpu.py::test_fused_sinkhorn_loop_equals_unfused[2-300-700]', {'B': 2, 'N': 300, 'M': 700}),
            ('tests/test_emd_gpu.py::test_fused_sinkhorn_loop_equals_unfused[5-2048-2048]', {'B': 5, 'N': 2048, 'M': 2048}),
            ('tests/test_emd_gpu.py::test_sinkhorn_vs_independent_float64', {'B': 2, 'N': 700, 'M': 600}),
        ],
    },
    {
        "entry": 'fpsg_sinkhorn_divergence_grad', "file": 'sinkhorn.hip',
        "kernel": 'sinkhorn_grad_kernel<2>',
        "lines": [
            'if (R == 2) hipLaunchKernelGGL((sinkhorn_grad_kernel<2>), grid, dim3(kSmThreads), 0, s, g);',
            'constexpr int kCUs = 256;',
            'inline int step_owners_per_lane(long workgroups_at_two) { return workgroups_at_two >= 4L * kCUs ? 2 : 1; }',
        ],
        "when": 'ceil(max(N, M) / 128) * 4 * B >= 1024',
        "cond": '-(-max(N, M) // 128) * 4 * B >= 4 * 256',
        "cases": [
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[two owners per lane, ragged 256x100x37]', {'B': 256, 'N': 100, 'M': 37}),
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[two owners per lane, ragged 256x70x129]', {'B': 256, 'N': 70, 'M': 129}),
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[two owners per lane, ragged 300x1x9]', {'B': 300, 'N': 1, 'M': 9}),
            ('tests/test_sinkhorn_grad_gpu.py::test_two_owners_per_lane_equal_one_owner_bit_for_bit[256-100-37]', {'B': 256, 'N': 100, 'M': 37}),
            ('tests/test_sinkhorn_grad_gpu.py::test_two_owners_per_lane_equal_one_owner_bit_for_bit[256-70-129]', {'B': 256, 'N': 70, 'M': 129}),
            ('tests/test_sinkhorn_grad_gpu.py::test_two_owners_per_lane_equal_one_owner_bit_for_bit[300-1-9]', {'B': 300, 'N': 1, 'M': 9}),
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[two owners per lane]', {'B': 64, 'N': 512, 'M': 512}),
        ],
    },
    {
        "entry": 'fpsg_sinkhorn_divergence_grad', "file": 'sinkhorn.hip',
        "kernel": 'sinkhorn_grad_kernel<1>',
        "lines": [
            'else hipLaunchKernelGGL((sinkhorn_grad_kernel<1>), grid, dim3(kSmThreads), 0, s, g);',
            'constexpr int kCUs = 256;',
            'inline int step_owners_per_lane(long workgroups_at_two) { return workgroups_at_two >= 4L * kCUs ? 2 : 1; }',
        ],
        "when": 'ceil(max(N, M) / 128) * 4 * B < 1024',
        "cond": 'not (-(-max(N, M) // 128) * 4 * B >= 4 * 256)',
        "cases": [
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[ragged 8-chunk]', {'B': 3, 'N': 300, 'M': 257}),
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[two LDS tiles]', {'B': 1, 'N': 2100, 'M': 520}),
            ('tests/test_sinkhorn_grad_gpu.py::test_gradient_against_float64[single owner]', {'B': 1, 'N': 1, 'M': 7}),
        ],
    },
    # ---- emd_cross.hip -------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_emd_cross', "file": 'emd_cross.hip',
        "kernel": 'emd_cross_kernel<4>',
        "lines": [
            'if (N <= 256) return launch_emd_cross<4>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status,',
        ],
        "when": 'N <= 256',
        "cond": 'N <= 256',
        "cases": [
            ('tests/test_emd_cross_gpu.py::test_against_hungarian', {'N': 256}),
            ('tests/test_emd_cross_gpu.py::test_hard_inputs', {'N': 256}),
            ('tests/test_emd_cross_gpu.py::test_load_balancing', {'N': 128}),
        ],
    },
    {
        "entry": 'fpsg_emd_cross', "file": 'emd_cross.hip',
        "kernel": 'emd_cross_kernel<8>',
        "lines": [
            'if (N <= 512) return launch_emd_cross<8>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status,',
        ],
        "when": '256 < N <= 512',
        "cond": '256 < N <= 512',
        "cases": [
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12[257]', {'N': 257}),
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12[300]', {'N': 300}),
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12[512]', {'N': 512}),
        ],
    },
    {
        "entry": 'fpsg_emd_cross', "file": 'emd_cross.hip',
        "kernel": 'emd_cross_kernel<16>',
        "lines": [
            'if (N <= 1024) return launch_emd_cross<16>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status,',
        ],
        "when": '512 < N <= 1024',
        "cond": '512 < N <= 1024',
        "cases": [
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12[513]', {'N': 513}),
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12[1024]', {'N': 1024}),
            ('tests/test_emd_cross_gpu.py::test_against_hungarian_n600', {'N': 600}),
        ],
    },
    {
        "entry": 'fpsg_emd_cross', "file": 'emd_cross.hip',
        "kernel": 'emd_cross_kernel<32>',
        "lines": [
            'return launch_emd_cross<32>(xyz1, xyz2, Na, Nb, N, eps_final, max_rounds, sym, cost, gap, status, rounds, counter,',
        ],
        "when": 'N > 1024',
        "cond": 'N > 1024',
        "cases": [
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12[1025]', {'N': 1025}),
            ('tests/test_emd_cross_gpu.py::test_same_trajectory_as_k12_n2048', {'N': 2048}),
        ],
    },
    # ---- expansion.hip -------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_expansion_fwd', "file": 'expansion.hip',
        "kernel": 'expansion_fwd_kernel<1>',
        "lines": [
            'if ((P) <= 64) { LAUNCH(1) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_FWD);',
        ],
        "when": 'P <= 64',
        "cond": 'P <= 64',
        "cases": [
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[2-3]', {'P': 2}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[3-3]', {'P': 3}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[63-3]', {'P': 63}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[64-3]', {'P': 64}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[64-1.0]', {'P': 64}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[64-1.5]', {'P': 64}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[64-2.0]', {'P': 64}),
        ],
    },
    {
        "entry": 'fpsg_expansion_bwd', "file": 'expansion.hip',
        "kernel": 'expansion_bwd_kernel<1>',
        "lines": [
            'if ((P) <= 64) { LAUNCH(1) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_BWD);',
        ],
        "when": 'P <= 64',
        "cond": 'P <= 64',
        "cases": [
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[64-1.0]', {'P': 64}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[64-1.5]', {'P': 64}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[64-2.0]', {'P': 64}),
        ],
    },
    {
        "entry": 'fpsg_expansion_fwd', "file": 'expansion.hip',
        "kernel": 'expansion_fwd_kernel<2>',
        "lines": [
            'else if ((P) <= 128) { LAUNCH(2) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_FWD);',
        ],
        "when": '64 < P <= 128',
        "cond": '64 < P <= 128',
        "cases": [
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[65-3]', {'P': 65}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[128-3]', {'P': 128}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[128-1.0]', {'P': 128}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[128-1.5]', {'P': 128}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[128-2.0]', {'P': 128}),
        ],
    },
    {
        "entry": 'fpsg_expansion_bwd', "file": 'expansion.hip',
        "kernel": 'expansion_bwd_kernel<2>',
        "lines": [
            'else if ((P) <= 128) { LAUNCH(2) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_BWD);',
        ],
        "when": '64 < P <= 128',
        "cond": '64 < P <= 128',
        "cases": [
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[128-1.0]', {'P': 128}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[128-1.5]', {'P': 128}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[128-2.0]', {'P': 128}),
        ],
    },
    {
        "entry": 'fpsg_expansion_fwd', "file": 'expansion.hip',
        "kernel": 'expansion_fwd_kernel<4>',
        "lines": [
            'else if ((P) <= 256) { LAUNCH(4) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_FWD);',
        ],
        "when": '128 < P <= 256',
        "cond": '128 < P <= 256',
        "cases": [
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[129-3]', {'P': 129}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[256-3]', {'P': 256}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[256-1.0]', {'P': 256}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[256-1.5]', {'P': 256}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[256-2.0]', {'P': 256}),
        ],
    },
    {
        "entry": 'fpsg_expansion_bwd', "file": 'expansion.hip',
        "kernel": 'expansion_bwd_kernel<4>',
        "lines": [
            'else if ((P) <= 256) { LAUNCH(4) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_BWD);',
        ],
        "when": '128 < P <= 256',
        "cond": '128 < P <= 256',
        "cases": [
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[256-1.0]', {'P': 256}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[256-1.5]', {'P': 256}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[256-2.0]', {'P': 256}),
        ],
    },
    {
        "entry": 'fpsg_expansion_fwd', "file": 'expansion.hip',
        "kernel": 'expansion_fwd_kernel<8>',
        "lines": [
            'else if ((P) <= 512) { LAUNCH(8) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_FWD);',
        ],
        "when": '256 < P <= 512',
        "cond": '256 < P <= 512',
        "cases": [
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[257-3]', {'P': 257}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[512-3]', {'P': 512}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[512-1.0]', {'P': 512}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[512-1.5]', {'P': 512}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[512-2.0]', {'P': 512}),
        ],
    },
    {
        "entry": 'fpsg_expansion_bwd', "file": 'expansion.hip',
        "kernel": 'expansion_bwd_kernel<8>',
        "lines": [
            'else if ((P) <= 512) { LAUNCH(8) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_BWD);',
        ],
        "when": '256 < P <= 512',
        "cond": '256 < P <= 512',
        "cases": [
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[512-1.0]', {'P': 512}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[512-1.5]', {'P': 512}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[512-2.0]', {'P': 512}),
        ],
    },
    {
        "entry": 'fpsg_expansion_fwd', "file": 'expansion.hip',
        "kernel": 'expansion_fwd_kernel<16>',
        "lines": [
            'else { LAUNCH(16) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_FWD);',
        ],
        "when": 'P > 512',
        "cond": 'P > 512',
        "cases": [
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[513-3]', {'P': 513}),
            ('tests/test_expansion_gpu.py::test_trees_equal_the_float64_prim_on_exact_distances[1024-2]', {'P': 1024}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[1024-1.0]', {'P': 1024}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[1024-1.5]', {'P': 1024}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[1024-2.0]', {'P': 1024}),
        ],
    },
    {
        "entry": 'fpsg_expansion_bwd', "file": 'expansion.hip',
        "kernel": 'expansion_bwd_kernel<16>',
        "lines": [
            'else { LAUNCH(16) }',
            'FPSG_EXP_DISPATCH(P, FPSG_EXP_BWD);',
        ],
        "when": 'P > 512',
        "cond": 'P > 512',
        "cases": [
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[1024-1.0]', {'P': 1024}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[1024-1.5]', {'P': 1024}),
            ('tests/test_expansion_gpu.py::test_value_and_gradient_against_float64[1024-2.0]', {'P': 1024}),
        ],
    },
    # ---- repulsion.hip -------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<1>',
        "lines": [
            'FPSG_REP_FWD(1) FPSG_REP_FWD(2) FPSG_REP_FWD(3) FPSG_REP_FWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 1',
        "cond": 'k == 1',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-1]', {'k': 1}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-1]', {'k': 1}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-1]', {'k': 1}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<1>',
        "lines": [
            'FPSG_REP_BWD(1) FPSG_REP_BWD(2) FPSG_REP_BWD(3) FPSG_REP_BWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 1',
        "cond": 'k == 1',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-1]', {'k': 1}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<2>',
        "lines": [
            'FPSG_REP_FWD(1) FPSG_REP_FWD(2) FPSG_REP_FWD(3) FPSG_REP_FWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 2',
        "cond": 'k == 2',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-2]', {'k': 2}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-2]', {'k': 2}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-2]', {'k': 2}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<2>',
        "lines": [
            'FPSG_REP_BWD(1) FPSG_REP_BWD(2) FPSG_REP_BWD(3) FPSG_REP_BWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 2',
        "cond": 'k == 2',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-2]', {'k': 2}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<3>',
        "lines": [
            'FPSG_REP_FWD(1) FPSG_REP_FWD(2) FPSG_REP_FWD(3) FPSG_REP_FWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 3',
        "cond": 'k == 3',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-3]', {'k': 3}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-3]', {'k': 3}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-3]', {'k': 3}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<3>',
        "lines": [
            'FPSG_REP_BWD(1) FPSG_REP_BWD(2) FPSG_REP_BWD(3) FPSG_REP_BWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 3',
        "cond": 'k == 3',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-3]', {'k': 3}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<4>',
        "lines": [
            'FPSG_REP_FWD(1) FPSG_REP_FWD(2) FPSG_REP_FWD(3) FPSG_REP_FWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 4',
        "cond": 'k == 4',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-4]', {'k': 4}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-4]', {'k': 4}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-4]', {'k': 4}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<4>',
        "lines": [
            'FPSG_REP_BWD(1) FPSG_REP_BWD(2) FPSG_REP_BWD(3) FPSG_REP_BWD(4)',
            'switch (k) {',
        ],
        "when": 'k == 4',
        "cond": 'k == 4',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-4]', {'k': 4}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<5>',
        "lines": [
            'FPSG_REP_FWD(5) FPSG_REP_FWD(6) FPSG_REP_FWD(7) FPSG_REP_FWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 5',
        "cond": 'k == 5',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-5]', {'k': 5}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-5]', {'k': 5}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-5]', {'k': 5}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<5>',
        "lines": [
            'FPSG_REP_BWD(5) FPSG_REP_BWD(6) FPSG_REP_BWD(7) FPSG_REP_BWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 5',
        "cond": 'k == 5',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-5]', {'k': 5}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<6>',
        "lines": [
            'FPSG_REP_FWD(5) FPSG_REP_FWD(6) FPSG_REP_FWD(7) FPSG_REP_FWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 6',
        "cond": 'k == 6',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-6]', {'k': 6}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-6]', {'k': 6}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-6]', {'k': 6}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<6>',
        "lines": [
            'FPSG_REP_BWD(5) FPSG_REP_BWD(6) FPSG_REP_BWD(7) FPSG_REP_BWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 6',
        "cond": 'k == 6',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-6]', {'k': 6}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<7>',
        "lines": [
            'FPSG_REP_FWD(5) FPSG_REP_FWD(6) FPSG_REP_FWD(7) FPSG_REP_FWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 7',
        "cond": 'k == 7',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-7]', {'k': 7}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-7]', {'k': 7}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-7]', {'k': 7}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<7>',
        "lines": [
            'FPSG_REP_BWD(5) FPSG_REP_BWD(6) FPSG_REP_BWD(7) FPSG_REP_BWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 7',
        "cond": 'k == 7',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-7]', {'k': 7}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_fwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_fwd_kernel<8>',
        "lines": [
            'FPSG_REP_FWD(5) FPSG_REP_FWD(6) FPSG_REP_FWD(7) FPSG_REP_FWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 8',
        "cond": 'k == 8',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[k+1-8]', {'k': 8}),
            ('tests/test_repulsion_gpu.py::test_lists_equal_the_float64_full_sort_on_exact_distances[65-8]', {'k': 8}),
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-8]', {'k': 8}),
        ],
    },
    {
        "entry": 'fpsg_repulsion_bwd', "file": 'repulsion.hip',
        "kernel": 'repulsion_bwd_kernel<8>',
        "lines": [
            'FPSG_REP_BWD(5) FPSG_REP_BWD(6) FPSG_REP_BWD(7) FPSG_REP_BWD(8)',
            'switch (k) {',
        ],
        "when": 'k == 8',
        "cond": 'k == 8',
        "cases": [
            ('tests/test_repulsion_gpu.py::test_value_and_gradient_against_float64[65-8]', {'k': 8}),
        ],
    },
    # ---- swd.hip -------------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_swd', "file": 'swd.hip',
        "kernel": 'swd_kernel<64>',
        "lines": [
            'if (N <= 64) FPSG_SWD_LAUNCH(64);',
        ],
        "when": 'N <= 64',
        "cond": 'N <= 64',
        "cases": [
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[1]', {'N': 1}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[1]', {'N': 1}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[1]', {'N': 1}),
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[3]', {'N': 3}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[3]', {'N': 3}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[3]', {'N': 3}),
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[64]', {'N': 64}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[64]', {'N': 64}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[64]', {'N': 64}),
        ],
    },
    {
        "entry": 'fpsg_swd', "file": 'swd.hip',
        "kernel": 'swd_kernel<128>',
        "lines": [
            'else if (N <= 128) FPSG_SWD_LAUNCH(128);',
        ],
        "when": '64 < N <= 128',
        "cond": '64 < N <= 128',
        "cases": [
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[65]', {'N': 65}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[65]', {'N': 65}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[65]', {'N': 65}),
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[128]', {'N': 128}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[128]', {'N': 128}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[128]', {'N': 128}),
        ],
    },
    {
        "entry": 'fpsg_swd', "file": 'swd.hip',
        "kernel": 'swd_kernel<256>',
        "lines": [
            'else if (N <= 256) FPSG_SWD_LAUNCH(256);',
        ],
        "when": '128 < N <= 256',
        "cond": '128 < N <= 256',
        "cases": [
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[129]', {'N': 129}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[129]', {'N': 129}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[129]', {'N': 129}),
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[256]', {'N': 256}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[256]', {'N': 256}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[256]', {'N': 256}),
        ],
    },
    {
        "entry": 'fpsg_swd', "file": 'swd.hip',
        "kernel": 'swd_kernel<512>',
        "lines": [
            'else if (N <= 512) FPSG_SWD_LAUNCH(512);',
        ],
        "when": '256 < N <= 512',
        "cond": '256 < N <= 512',
        "cases": [
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[257]', {'N': 257}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[257]', {'N': 257}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[257]', {'N': 257}),
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[512]', {'N': 512}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[512]', {'N': 512}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[512]', {'N': 512}),
        ],
    },
    {
        "entry": 'fpsg_swd', "file": 'swd.hip',
        "kernel": 'swd_kernel<1024>',
        "lines": [
            'else if (N <= 1024) FPSG_SWD_LAUNCH(1024);',
        ],
        "when": '512 < N <= 1024',
        "cond": '512 < N <= 1024',
        "cases": [
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[513]', {'N': 513}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[513]', {'N': 513}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[513]', {'N': 513}),
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[1024]', {'N': 1024}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[1024]', {'N': 1024}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[1024]', {'N': 1024}),
        ],
    },
    {
        "entry": 'fpsg_swd', "file": 'swd.hip',
        "kernel": 'swd_kernel<2048>',
        "lines": [
            'else FPSG_SWD_LAUNCH(2048);',
        ],
        "when": 'N > 1024',
        "cond": 'N > 1024',
        "cases": [
            ('tests/test_swd_gpu.py::test_sort_is_the_references_order_element_for_element[2048]', {'N': 2048}),
            ('tests/test_swd_gpu.py::test_value_and_gradient_against_the_fp32_key_reference[2048]', {'N': 2048}),
            ('tests/test_swd_gpu.py::test_value_against_float64_keys[2048]', {'N': 2048}),
        ],
    },
    # ---- uniform.hip ---------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_uniform_fwd', "file": 'uniform.hip',
        "kernel": 'uniform_fwd_kernel<1>',
        "lines": [
            'if (cap == 64) { FPSG_UNI_FWD(1) }',
        ],
        "when": 'cap == 64',
        "cond": 'cap == 64',
        "cases": [
            ('tests/test_uniform_gpu.py::test_caps_retain_the_first_members_in_index_order', {'cap': 64}),
            ('tests/test_uniform_gpu.py::test_lists_equal_the_float64_computation_on_exact_distances[257-7]', {'cap': 64}),
            ('tests/test_uniform_gpu.py::test_value_and_gradient_against_float64_at_every_cap[64]', {'cap': 64}),
        ],
    },
    {
        "entry": 'fpsg_uniform_fwd', "file": 'uniform.hip',
        "kernel": 'uniform_fwd_kernel<2>',
        "lines": [
            'else if (cap == 128) { FPSG_UNI_FWD(2) }',
        ],
        "when": 'cap == 128',
        "cond": 'cap == 128',
        "cases": [
            ('tests/test_uniform_gpu.py::test_caps_retain_the_first_members_in_index_order', {'cap': 128}),
            ('tests/test_uniform_gpu.py::test_value_and_gradient_against_float64_at_every_cap[128]', {'cap': 128}),
        ],
    },
    {
        "entry": 'fpsg_uniform_fwd', "file": 'uniform.hip',
        "kernel": 'uniform_fwd_kernel<4>',
        "lines": [
            'else { FPSG_UNI_FWD(4) }',
        ],
        "when": 'cap == 256',
        "cond": 'cap == 256',
        "cases": [
            ('tests/test_uniform_gpu.py::test_caps_retain_the_first_members_in_index_order', {'cap': 256}),
            ('tests/test_uniform_gpu.py::test_value_and_gradient_against_float64_at_every_cap[256]', {'cap': 256}),
        ],
    },
    # ---- point_normals.hip ---------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_point_normals', "file": 'point_normals.hip',
        "kernel": 'pn_select_kernel<8>',
        "lines": [
            'if (k <= 8) hipLaunchKernelGGL(pn_select_kernel<8>, grid, dim3(kPnThreads), 0, s, xyz, N, k, lists);',
        ],
        "when": 'k <= 8',
        "cond": 'k <= 8',
        "cases": [
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[1-4-3]', {'k': 3}),
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[3-63-8]', {'k': 8}),
        ],
    },
    {
        "entry": 'fpsg_point_normals', "file": 'point_normals.hip',
        "kernel": 'pn_select_kernel<16>',
        "lines": [
            'else if (k <= 16) hipLaunchKernelGGL(pn_select_kernel<16>, grid, dim3(kPnThreads), 0, s, xyz, N, k, lists);',
        ],
        "when": '8 < k <= 16',
        "cond": '8 < k <= 16',
        "cases": [
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[2-70-9]', {'k': 9}),
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[3-64-16]', {'k': 16}),
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[2-257-16]', {'k': 16}),
        ],
    },
    {
        "entry": 'fpsg_point_normals', "file": 'point_normals.hip',
        "kernel": 'pn_select_kernel<32>',
        "lines": [
            'else hipLaunchKernelGGL(pn_select_kernel<32>, grid, dim3(kPnThreads), 0, s, xyz, N, k, lists);',
        ],
        "when": 'k > 16',
        "cond": 'k > 16',
        "cases": [
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[2-70-17]', {'k': 17}),
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[2-65-32]', {'k': 32}),
            ('tests/test_point_normals_gpu.py::test_lists_equal_the_restatement[1-33-32]', {'k': 32}),
        ],
    },
    # ---- views.hip -----------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_episode_views', "file": 'views.hip',
        "kernel": 'episode_views_kernel<4>',
        "lines": [
            'if (wide)',
            'const bool wide = Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;',
        ],
        "when": 'Wo a multiple of 4 and out 16-byte aligned',
        "cond": 'Wo % 4 == 0',
        "cases": [
            ('tests/test_views_gpu.py::test_equals_the_restatement_bit_for_bit[shape0-size0]', {'Wo': 4}),
            ('tests/test_views_gpu.py::test_equals_the_restatement_bit_for_bit[shape1-size1]', {'Wo': 8}),
            ('tests/test_views_gpu.py::test_equals_the_restatement_bit_for_bit[shape0-size3]', {'Wo': 12}),
        ],
    },
    {
        "entry": 'fpsg_episode_views', "file": 'views.hip',
        "kernel": 'episode_views_kernel<1>',
        "lines": [
            'hipLaunchKernelGGL(episode_views_kernel<1>, grid, dim3(kThreads), 0, st, src, n_src, Hs, Ws, sel, geom, color, out,',
            'const bool wide = Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;',
        ],
        "when": 'otherwise',
        "cond": 'Wo % 4 != 0',
        "cases": [
            ('tests/test_views_gpu.py::test_equals_the_restatement_bit_for_bit[shape0-size2]', {'Wo': 5}),
            ('tests/test_views_gpu.py::test_equals_the_restatement_bit_for_bit[shape1-size2]', {'Wo': 5}),
        ],
    },
    # ---- points_render.hip ---------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_points_render', "file": 'points_render.hip',
        "kernel": 'points_tile_kernel<true>',
        "lines": [
            'if (colors)',
        ],
        "when": 'colors given',
        "cond": None,
        "cases": [
            ('tests/test_points_render_gpu.py::test_radiance_against_float64_within_the_derived_bound[2-True]', None),
            ('tests/test_points_render_gpu.py::test_two_clouds_one_point_past_a_chunk_three_views[True]', None),
        ],
    },
    {
        "entry": 'fpsg_points_render', "file": 'points_render.hip',
        "kernel": 'points_tile_kernel<false>',
        "lines": [
            'hipLaunchKernelGGL(points_tile_kernel<false>, grid, dim3(kThreads), 0, st, rec, N, W, H, ssaa, R, radius, Q,',
        ],
        "when": 'colors == NULL',
        "cond": None,
        "cases": [
            ('tests/test_points_render_gpu.py::test_radiance_against_float64_within_the_derived_bound[1-False]', None),
            ('tests/test_points_render_gpu.py::test_radiance_against_float64_within_the_derived_bound[4-False]', None),
            ('tests/test_points_render_gpu.py::test_two_clouds_one_point_past_a_chunk_three_views[False]', None),
        ],
    },
    # ---- knn.hip -------------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<8, 1, 16, false>',
        "lines": [
            'if (C <= 4) return launch_knn<VPL, 1, 16>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 8) return launch_knn_c<8>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N <= 512 and C <= 4',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 <= 8) and (C <= 4)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-16-5]', {'C': 3, 'N': 16}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-3-129-20]', {'C': 3, 'N': 129}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-1-257-3]', {'C': 1, 'N': 257}),
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[3-3-33-33]', {'C': 3, 'N': 33}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<16, 1, 16, false>',
        "lines": [
            'if (C <= 4) return launch_knn<VPL, 1, 16>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 16) return launch_knn_c<16>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '512 < N <= 1024 and C <= 4',
        "cond": '(8 < ((N + 15) // 16 * 16 + 63) // 64 <= 16) and (C <= 4)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-513-7]', {'C': 3, 'N': 513}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[3-3-1024-24]', {'C': 3, 'N': 1024}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-4-700-24]', {'C': 4, 'N': 700}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<32, 1, 16, false>',
        "lines": [
            'if (C <= 4) return launch_knn<VPL, 1, 16>(x, xx, nullptr, B, C, N, k, idx, s);',
            'return launch_knn_c<32>(x, xx, xk, B, C, N, k, idx, s);   // N > 2048: chunks of 2048 columns',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N > 1024 and C <= 4',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 > 16) and (C <= 4)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-2-2048-20]', {'C': 2, 'N': 2048}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<8, 16, 16, true>',
        "lines": [
            'if (xk && C > 32 && C <= 64) return launch_knn<VPL, 16, 16, true>(x, xx, xk, B, C, N, k, idx, s);',
            'if (vpl <= 8) return launch_knn_c<8>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N <= 512 and 32 < C <= 64 and C % 16 == 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 <= 8) and (32 < C <= 64 and C % 16 == 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-64-64-20]', {'C': 64, 'N': 64}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-48-257-9]', {'C': 48, 'N': 257}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[10-64-256-20]', {'C': 64, 'N': 256}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<16, 16, 16, true>',
        "lines": [
            'if (xk && C > 32 && C <= 64) return launch_knn<VPL, 16, 16, true>(x, xx, xk, B, C, N, k, idx, s);',
            'if (vpl <= 16) return launch_knn_c<16>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '512 < N <= 1024 and 32 < C <= 64 and C % 16 == 0',
        "cond": '(8 < ((N + 15) // 16 * 16 + 63) // 64 <= 16) and (32 < C <= 64 and C % 16 == 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-64-1000-20]', {'C': 64, 'N': 1000}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<32, 16, 16, true>',
        "lines": [
            'if (xk && C > 32 && C <= 64) return launch_knn<VPL, 16, 16, true>(x, xx, xk, B, C, N, k, idx, s);',
            'return launch_knn_c<32>(x, xx, xk, B, C, N, k, idx, s);   // N > 2048: chunks of 2048 columns',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N > 1024 and 32 < C <= 64 and C % 16 == 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 > 16) and (32 < C <= 64 and C % 16 == 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[1-64-4100-32]', {'C': 64, 'N': 4100}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<8, 32, 8, true>',
        "lines": [
            'if (xk && C > 64 && C <= 128) return launch_knn<VPL, 32, 8, true>(x, xx, xk, B, C, N, k, idx, s);',
            'if (vpl <= 8) return launch_knn_c<8>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N <= 512 and 64 < C <= 128 and C % 16 == 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 <= 8) and (64 < C <= 128 and C % 16 == 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-128-33-20]', {'C': 128, 'N': 33}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-128-200-13]', {'C': 128, 'N': 200}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<16, 32, 8, true>',
        "lines": [
            'if (xk && C > 64 && C <= 128) return launch_knn<VPL, 32, 8, true>(x, xx, xk, B, C, N, k, idx, s);',
            'if (vpl <= 16) return launch_knn_c<16>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '512 < N <= 1024 and 64 < C <= 128 and C % 16 == 0',
        "cond": '(8 < ((N + 15) // 16 * 16 + 63) // 64 <= 16) and (64 < C <= 128 and C % 16 == 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-128-600-9]', {'C': 128, 'N': 600}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<32, 32, 8, true>',
        "lines": [
            'if (xk && C > 64 && C <= 128) return launch_knn<VPL, 32, 8, true>(x, xx, xk, B, C, N, k, idx, s);',
            'return launch_knn_c<32>(x, xx, xk, B, C, N, k, idx, s);   // N > 2048: chunks of 2048 columns',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N > 1024 and 64 < C <= 128 and C % 16 == 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 > 16) and (64 < C <= 128 and C % 16 == 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-80-1040-9]', {'C': 80, 'N': 1040}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<8, 16, 16, false>',
        "lines": [
            'if (C > 32 && C <= 64) return launch_knn<VPL, 16, 16>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 8) return launch_knn_c<8>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N <= 512 and 32 < C <= 64 and C % 16 != 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 <= 8) and (32 < C <= 64 and C % 16 != 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-40-65-9]', {'C': 40, 'N': 65}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<16, 16, 16, false>',
        "lines": [
            'if (C > 32 && C <= 64) return launch_knn<VPL, 16, 16>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 16) return launch_knn_c<16>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '512 < N <= 1024 and 32 < C <= 64 and C % 16 != 0',
        "cond": '(8 < ((N + 15) // 16 * 16 + 63) // 64 <= 16) and (32 < C <= 64 and C % 16 != 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-40-600-9]', {'C': 40, 'N': 600}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<32, 16, 16, false>',
        "lines": [
            'if (C > 32 && C <= 64) return launch_knn<VPL, 16, 16>(x, xx, nullptr, B, C, N, k, idx, s);',
            'return launch_knn_c<32>(x, xx, xk, B, C, N, k, idx, s);   // N > 2048: chunks of 2048 columns',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N > 1024 and 32 < C <= 64 and C % 16 != 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 > 16) and (32 < C <= 64 and C % 16 != 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-40-1040-9]', {'C': 40, 'N': 1040}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<8, 32, 8, false>',
        "lines": [
            'if (C > 64 && C <= 128) return launch_knn<VPL, 32, 8>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 8) return launch_knn_c<8>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N <= 512 and 64 < C <= 128 and C % 16 != 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 <= 8) and (64 < C <= 128 and C % 16 != 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-100-130-9]', {'C': 100, 'N': 130}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<16, 32, 8, false>',
        "lines": [
            'if (C > 64 && C <= 128) return launch_knn<VPL, 32, 8>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 16) return launch_knn_c<16>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '512 < N <= 1024 and 64 < C <= 128 and C % 16 != 0',
        "cond": '(8 < ((N + 15) // 16 * 16 + 63) // 64 <= 16) and (64 < C <= 128 and C % 16 != 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-100-777-20]', {'C': 100, 'N': 777}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<32, 32, 8, false>',
        "lines": [
            'if (C > 64 && C <= 128) return launch_knn<VPL, 32, 8>(x, xx, nullptr, B, C, N, k, idx, s);',
            'return launch_knn_c<32>(x, xx, xk, B, C, N, k, idx, s);   // N > 2048: chunks of 2048 columns',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N > 1024 and 64 < C <= 128 and C % 16 != 0',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 > 16) and (64 < C <= 128 and C % 16 != 0)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-100-1040-9]', {'C': 100, 'N': 1040}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<8, 0, 8, false>',
        "lines": [
            'return launch_knn<VPL, 0, 8>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 8) return launch_knn_c<8>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N <= 512 and 4 < C <= 32 or C > 128',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 <= 8) and (4 < C <= 32 or C > 128)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[1-130-300-16]', {'C': 130, 'N': 300}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<16, 0, 8, false>',
        "lines": [
            'return launch_knn<VPL, 0, 8>(x, xx, nullptr, B, C, N, k, idx, s);',
            'if (vpl <= 16) return launch_knn_c<16>(x, xx, xk, B, C, N, k, idx, s);',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '512 < N <= 1024 and 4 < C <= 32 or C > 128',
        "cond": '(8 < ((N + 15) // 16 * 16 + 63) // 64 <= 16) and (4 < C <= 32 or C > 128)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-17-600-9]', {'C': 17, 'N': 600}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<32, 0, 8, false>',
        "lines": [
            'return launch_knn<VPL, 0, 8>(x, xx, nullptr, B, C, N, k, idx, s);',
            'return launch_knn_c<32>(x, xx, xk, B, C, N, k, idx, s);   // N > 2048: chunks of 2048 columns',
            'const int vpl = (((N + 15) / 16) * 16 + 63) / 64;',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'N > 1024 and 4 < C <= 32 or C > 128',
        "cond": '(((N + 15) // 16 * 16 + 63) // 64 > 16) and (4 < C <= 32 or C > 128)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-17-2048-20]', {'C': 17, 'N': 2048}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_prep_kernel',
        "lines": [
            'if (knn_uses_pm(C) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0) {',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": '33..128 channels, a multiple of 16, workspace 16-byte aligned',
        "cond": 'C % 16 == 0 and 32 < C <= 128',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-48-257-9]', {'C': 48, 'N': 257}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-128-600-9]', {'C': 128, 'N': 600}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-80-1040-9]', {'C': 80, 'N': 1040}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'sqnorm_kernel',
        "lines": [
            'hipLaunchKernelGGL(sqnorm_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, x, C, N, xx);',
            'inline bool knn_uses_pm(int C) { return C % 16 == 0 && C > 32 && C <= 128; }',
        ],
        "when": 'otherwise',
        "cond": 'not (C % 16 == 0 and 32 < C <= 128)',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-16-5]', {'C': 3, 'N': 16}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-40-600-9]', {'C': 40, 'N': 600}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-100-777-20]', {'C': 100, 'N': 777}),
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[1-130-300-16]', {'C': 130, 'N': 300}),
        ],
    },
    # ---- winograd.hip --------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_wino_input_transform', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, false, true, false, false>',
        "lines": [
            'else if (beyond_cache((size_t)36 * C * Ps * sizeof(float))) hipLaunchKernelGGL((wino_input_kernel<4, false, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr);',
        ],
        "when": 'm = 4 and 36 C Ps floats beyond 300 MiB',
        "cond": '36 * C * 37 * (-(-H // 4)) ** 2 * 4 > 300 << 20',
        "cases": [
            ('tests/test_winograd_gpu.py::test_full_size_layers_against_the_library_and_linearity[layer2]', {'C': 128, 'H': 112}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, false, false, true, false>',
        "lines": [
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_output_kernel<4, false, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, nullptr, nullptr);',
        ],
        "when": 'm = 4 and 36 K Ps floats beyond 300 MiB',
        "cond": '36 * K * 37 * (-(-H // 4)) ** 2 * 4 > 300 << 20',
        "cases": [
            ('tests/test_winograd_gpu.py::test_full_size_layers_against_the_library_and_linearity[layer2]', {'K': 128, 'H': 112}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_transforms', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, false, true, false, true>',
        "lines": [
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_input_kernel<4, false, true, false, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr, dM);',
        ],
        "when": 'm = 4 and 36 K Ps floats beyond 300 MiB',
        "cond": '36 * K * 37 * (-(-H // 4)) ** 2 * 4 > 300 << 20',
        "cases": [
            ('tests/test_winograd_gpu.py::test_full_size_layers_against_the_library_and_linearity[layer2]', {'K': 128, 'H': 112}),
        ],
    },
    # ---- edgeconv.hip --------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_edgeconv_fwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_fwd_grouped_kernel<16>',
        "lines": [
            'if (Co == 64 && !one) hipLaunchKernelGGL(edgeconv_fwd_grouped_kernel<16>, grid, dim3(kEcThreads), 0, s, PQ, idx, sgn, B, N, k, bpc, ppw, ysel, jsel, s1, part);',
            'const bool one = edgeconv_bwd_one_edge();       // FPSG_EDGECONV_BWD=one_edge also selects the one-neighbour forward',
        ],
        "when": 'Co = 64, the grouped form (default)',
        "cond": 'Co == 64 and not one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B2-N300-k20-Co64-random-grouped]', {'Co': 64, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B1-N50-k64-Co64-degrees-grouped]', {'Co': 64, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B3-N7-k3-Co64-hubs-grouped]', {'Co': 64, 'one': False}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_fwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_fwd_grouped_kernel<32>',
        "lines": [
            'else if (Co == 128 && !one) hipLaunchKernelGGL(edgeconv_fwd_grouped_kernel<32>, grid, dim3(kEcThreads), 0, s, PQ, idx, sgn, B, N, k, bpc, ppw, ysel, jsel, s1, part);',
            'const bool one = edgeconv_bwd_one_edge();       // FPSG_EDGECONV_BWD=one_edge also selects the one-neighbour forward',
        ],
        "when": 'Co = 128, the grouped form (default)',
        "cond": 'Co == 128 and not one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B2-N300-k20-Co128-random-grouped]', {'Co': 128, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B1-N50-k64-Co128-degrees-grouped]', {'Co': 128, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B3-N7-k3-Co128-hubs-grouped]', {'Co': 128, 'one': False}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_fwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_fwd_kernel<1>',
        "lines": [
            'else if (Co == 64) hipLaunchKernelGGL(edgeconv_fwd_kernel<1>, grid, dim3(kEcThreads), 0, s, PQ, idx, sgn, B, N, k, bpc, ppw, ysel, jsel, s1, part);',
            'const bool one = edgeconv_bwd_one_edge();       // FPSG_EDGECONV_BWD=one_edge also selects the one-neighbour forward',
        ],
        "when": 'Co = 64, FPSG_EDGECONV_BWD=one_edge',
        "cond": 'Co == 64 and one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B2-N300-k20-Co64-random-one_edge]', {'Co': 64, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B1-N50-k64-Co64-degrees-one_edge]', {'Co': 64, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B3-N7-k3-Co64-hubs-one_edge]', {'Co': 64, 'one': True}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_fwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_fwd_kernel<2>',
        "lines": [
            'else if (Co == 128) hipLaunchKernelGGL(edgeconv_fwd_kernel<2>, grid, dim3(kEcThreads), 0, s, PQ, idx, sgn, B, N, k, bpc, ppw, ysel, jsel, s1, part);',
            'const bool one = edgeconv_bwd_one_edge();       // FPSG_EDGECONV_BWD=one_edge also selects the one-neighbour forward',
        ],
        "when": 'Co = 128, FPSG_EDGECONV_BWD=one_edge',
        "cond": 'Co == 128 and one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B2-N300-k20-Co128-random-one_edge]', {'Co': 128, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B1-N50-k64-Co128-degrees-one_edge]', {'Co': 128, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B3-N7-k3-Co128-hubs-one_edge]', {'Co': 128, 'one': True}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_fwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_fwd_kernel<4>',
        "lines": [
            'else hipLaunchKernelGGL(edgeconv_fwd_kernel<4>, grid, dim3(kEcThreads), 0, s, PQ, idx, sgn, B, N, k, bpc, ppw, ysel, jsel, s1, part);',
            'const bool one = edgeconv_bwd_one_edge();       // FPSG_EDGECONV_BWD=one_edge also selects the one-neighbour forward',
        ],
        "when": 'Co = 256, either form',
        "cond": 'Co == 256',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B2-N300-k20-Co256-random-grouped]', {'Co': 256, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B1-N50-k64-Co256-degrees-grouped]', {'Co': 256, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B3-N7-k3-Co256-hubs-grouped]', {'Co': 256, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B2-N300-k20-Co256-random-one_edge]', {'Co': 256, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B1-N50-k64-Co256-degrees-one_edge]', {'Co': 256, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_forward_kernel_is_exact_and_its_sums_are_within_fp32_bounds[B3-N7-k3-Co256-hubs-one_edge]', {'Co': 256, 'one': True}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_bwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_bwd_kernel<1>',
        "lines": [
            'if (Co == 64) hipLaunchKernelGGL(edgeconv_bwd_kernel<1>, grid, dim3(kEcThreads), 0, s, dzs, jsel, PQ, s1, rev, off, coef, B, N, k, bpc, ppw, nsl, stats, dPQ);',
            "if (edgeconv_bwd_one_edge()) {      // FPSG_EDGECONV_BWD=one_edge: round 2's form, one in-edge per load (A/B timing)",
        ],
        "when": 'Co = 64, FPSG_EDGECONV_BWD=one_edge',
        "cond": 'Co == 64 and one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B2-N300-k20-Co64-random-train-one_edge]', {'Co': 64, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B1-N50-k64-Co64-degrees-eval-one_edge]', {'Co': 64, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B3-N7-k3-Co64-hubs-train-one_edge]', {'Co': 64, 'one': True}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_bwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_bwd_kernel<2>',
        "lines": [
            'else hipLaunchKernelGGL(edgeconv_bwd_kernel<2>, grid, dim3(kEcThreads), 0, s, dzs, jsel, PQ, s1, rev, off, coef, B, N, k, bpc, ppw, nsl, stats, dPQ);',
            "if (edgeconv_bwd_one_edge()) {      // FPSG_EDGECONV_BWD=one_edge: round 2's form, one in-edge per load (A/B timing)",
            'const int nsl = Co == 256 ? 2 : 1;',
        ],
        "when": 'Co = 128 or 256 (two channel slices), FPSG_EDGECONV_BWD=one_edge',
        "cond": 'Co != 64 and one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B2-N300-k20-Co128-random-train-one_edge]', {'Co': 128, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B1-N50-k64-Co128-degrees-eval-one_edge]', {'Co': 128, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B3-N7-k3-Co128-hubs-train-one_edge]', {'Co': 128, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B2-N300-k20-Co256-random-train-one_edge]', {'Co': 256, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B1-N50-k64-Co256-degrees-eval-one_edge]', {'Co': 256, 'one': True}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B3-N7-k3-Co256-hubs-train-one_edge]', {'Co': 256, 'one': True}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_bwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_bwd_grouped_kernel<16>',
        "lines": [
            'if (Co == 64) hipLaunchKernelGGL(edgeconv_bwd_grouped_kernel<16>, grid, dim3(kEcThreads), 0, s, dzs, jsel, PQ, s1, rev, off, coef, B, N, k, bpc, ppw, nsl, stats, dPQ);',
            "if (edgeconv_bwd_one_edge()) {      // FPSG_EDGECONV_BWD=one_edge: round 2's form, one in-edge per load (A/B timing)",
        ],
        "when": 'Co = 64, the grouped form (default)',
        "cond": 'Co == 64 and not one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B2-N300-k20-Co64-random-train-grouped]', {'Co': 64, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B1-N50-k64-Co64-degrees-eval-grouped]', {'Co': 64, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B3-N7-k3-Co64-hubs-train-grouped]', {'Co': 64, 'one': False}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_bwd', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_bwd_grouped_kernel<32>',
        "lines": [
            'else hipLaunchKernelGGL(edgeconv_bwd_grouped_kernel<32>, grid, dim3(kEcThreads), 0, s, dzs, jsel, PQ, s1, rev, off, coef, B, N, k, bpc, ppw, nsl, stats, dPQ);',
            "if (edgeconv_bwd_one_edge()) {      // FPSG_EDGECONV_BWD=one_edge: round 2's form, one in-edge per load (A/B timing)",
            'const int nsl = Co == 256 ? 2 : 1;',
        ],
        "when": 'Co = 128 or 256 (two channel slices), the grouped form (default)',
        "cond": 'Co != 64 and not one',
        "cases": [
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B2-N300-k20-Co128-random-train-grouped]', {'Co': 128, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B1-N50-k64-Co128-degrees-eval-grouped]', {'Co': 128, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B3-N7-k3-Co128-hubs-train-grouped]', {'Co': 128, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B2-N300-k20-Co256-random-train-grouped]', {'Co': 256, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B1-N50-k64-Co256-degrees-eval-grouped]', {'Co': 256, 'one': False}),
            ('tests/test_edgeconv_gpu.py::test_backward_kernel_against_the_per_edge_definition[B3-N7-k3-Co256-hubs-train-grouped]', {'Co': 256, 'one': False}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_stats_finalize_ws', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_stats_finalize_kernel',
        "lines": [
            'if (!training || ws == nullptr || blocks < 256)       // nothing to sum / few rows: the one-launch form',
        ],
        "when": 'evaluation, no workspace, or fewer than 256 partial rows: the one-launch form',
        "cond": 'blocks < 256',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_edgeconv_statistics_finalize_in_two_stages[64-128]', {'blocks': 64}),
        ],
    },
    {
        "entry": 'fpsg_edgeconv_stats_finalize_ws', "file": 'edgeconv.hip',
        "kernel": 'edgeconv_stats_slices_kernel',
        "lines": [
            'hipLaunchKernelGGL(edgeconv_stats_slices_kernel, dim3((unsigned)Z, (unsigned)((2 * Co + kS1Cols - 1) / kS1Cols)), dim3(kS1Threads), 0,',
            'if (!training || ws == nullptr || blocks < 256)       // nothing to sum / few rows: the one-launch form',
        ],
        "when": 'training with a workspace and at least 256 partial rows: slice sums, then one wave per channel',
        "cond": 'blocks >= 256',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_edgeconv_statistics_finalize_in_two_stages[257-256]', {'blocks': 257}),
            ('tests/test_dgcnn_gpu.py::test_edgeconv_statistics_finalize_in_two_stages[300-64]', {'blocks': 300}),
            ('tests/test_dgcnn_gpu.py::test_edgeconv_statistics_finalize_in_two_stages[8192-128]', {'blocks': 8192}),
        ],
    },
    # ---- gemm_split.hip ------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 256, 16, 2, 4, 2, false, false,',
        "lines": [
            'case 0: FPSG_GEMM_LAUNCH(256, 256, 16, 2, 4, 2, false); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 0 (variant % 10 == 0, or the automatic choice), B as given',
        "cond": 'variant % 10 == 0 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-0]', {'variant': 0, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-0]', {'variant': 0, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-0]', {'variant': 0, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 256, 16, 2, 4, 2, true, false,',
        "lines": [
            'case 0: FPSG_GEMM_LAUNCH(256, 256, 16, 2, 4, 2, false); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 0 (variant % 10 == 0, or the automatic choice), B transposed',
        "cond": 'variant % 10 == 0 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-0]', {'variant': 0, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-20]', {'variant': 20, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-0]', {'variant': 0, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-512-512-7252--1]', None),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 128, 32, 2, 4, 2, false, false,',
        "lines": [
            'case 1: FPSG_GEMM_LAUNCH(256, 128, 32, 2, 4, 2, false); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 1 (variant % 10 == 1), B as given',
        "cond": 'variant % 10 == 1 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-1]', {'variant': 1, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-1]', {'variant': 1, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-1]', {'variant': 1, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 128, 32, 2, 4, 2, true, false,',
        "lines": [
            'case 1: FPSG_GEMM_LAUNCH(256, 128, 32, 2, 4, 2, false); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 1 (variant % 10 == 1), B transposed',
        "cond": 'variant % 10 == 1 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-1]', {'variant': 1, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-31]', {'variant': 31, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-1]', {'variant': 1, 'transB': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 128, 16, 2, 2, 3, false, false,',
        "lines": [
            'case 2: FPSG_GEMM_LAUNCH(128, 128, 16, 2, 2, 3, false); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 2 (variant % 10 == 2), B as given',
        "cond": 'variant % 10 == 2 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-2]', {'variant': 2, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-2]', {'variant': 2, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-2]', {'variant': 2, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 128, 16, 2, 2, 3, true, false,',
        "lines": [
            'case 2: FPSG_GEMM_LAUNCH(128, 128, 16, 2, 2, 3, false); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 2 (variant % 10 == 2), B transposed',
        "cond": 'variant % 10 == 2 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-2]', {'variant': 2, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-52]', {'variant': 52, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-2]', {'variant': 2, 'transB': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 256, 16, 1, 4, 2, false, false,',
        "lines": [
            'case 3: FPSG_GEMM_LAUNCH(128, 256, 16, 1, 4, 2, false); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 3 (variant % 10 == 3), B as given',
        "cond": 'variant % 10 == 3 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-3]', {'variant': 3, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-3]', {'variant': 3, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-3]', {'variant': 3, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 256, 16, 1, 4, 2, true, false,',
        "lines": [
            'case 3: FPSG_GEMM_LAUNCH(128, 256, 16, 1, 4, 2, false); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 3 (variant % 10 == 3), B transposed',
        "cond": 'variant % 10 == 3 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-3]', {'variant': 3, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-73]', {'variant': 73, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-3]', {'variant': 3, 'transB': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 256, 16, 2, 4, 2, false, true,',
        "lines": [
            'case 4: FPSG_GEMM_LAUNCH(256, 256, 16, 2, 4, 2, true); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 4 (variant % 10 == 4), B as given',
        "cond": 'variant % 10 == 4 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-4]', {'variant': 4, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-4]', {'variant': 4, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-4]', {'variant': 4, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 256, 16, 2, 4, 2, true, true,',
        "lines": [
            'case 4: FPSG_GEMM_LAUNCH(256, 256, 16, 2, 4, 2, true); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 4 (variant % 10 == 4), B transposed',
        "cond": 'variant % 10 == 4 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-4]', {'variant': 4, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-24]', {'variant': 24, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-4]', {'variant': 4, 'transB': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 128, 16, 2, 2, 3, false, true,',
        "lines": [
            'case 5: FPSG_GEMM_LAUNCH(128, 128, 16, 2, 2, 3, true); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 5 (variant % 10 == 5, or the automatic choice), B as given',
        "cond": 'variant % 10 == 5 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-5]', {'variant': 5, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-5]', {'variant': 5, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-5]', {'variant': 5, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48--1]', None),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 128, 16, 2, 2, 3, true, true,',
        "lines": [
            'case 5: FPSG_GEMM_LAUNCH(128, 128, 16, 2, 2, 3, true); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 5 (variant % 10 == 5, or the automatic choice), B transposed',
        "cond": 'variant % 10 == 5 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-5]', {'variant': 5, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-35]', {'variant': 35, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-5]', {'variant': 5, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53--1]', None),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 256, 16, 1, 4, 2, false, true,',
        "lines": [
            'case 6: FPSG_GEMM_LAUNCH(128, 256, 16, 1, 4, 2, true); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 6 (variant % 10 == 6), B as given',
        "cond": 'variant % 10 == 6 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-6]', {'variant': 6, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-6]', {'variant': 6, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-6]', {'variant': 6, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 256, 16, 1, 4, 2, true, true,',
        "lines": [
            'case 6: FPSG_GEMM_LAUNCH(128, 256, 16, 1, 4, 2, true); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 6 (variant % 10 == 6), B transposed',
        "cond": 'variant % 10 == 6 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-6]', {'variant': 6, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-46]', {'variant': 46, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-6]', {'variant': 6, 'transB': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 128, 16, 2, 4, 4, false, true,',
        "lines": [
            'default: FPSG_GEMM_LAUNCH(256, 128, 16, 2, 4, 4, true); break;',
            'else hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, false, PIPE>), grid, block, 0, s, g);        \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 7 (variant % 10 == 7), B as given',
        "cond": 'variant % 10 == 7 and transB == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-256-300-32-7]', {'variant': 7, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[3-100-70-48-7]', {'variant': 7, 'transB': 0}),
            ('tests/test_gemm_split_gpu.py::test_nn_matches_float64[2-37-1000-64-7]', {'variant': 7, 'transB': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<256, 128, 16, 2, 4, 4, true, true,',
        "lines": [
            'default: FPSG_GEMM_LAUNCH(256, 128, 16, 2, 4, 4, true); break;',
            'if (transB) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, BK, WR, WC, MINW, true, PIPE>), grid, block, 0, s, g);  \\',
            'if (tile < 0) tile = (transB && M >= 256 && N >= 256 && K >= 1024) ? 0 : 5;',
            'int tile = variant < 0 ? -1 : variant % 10;',
        ],
        "when": 'tile 7 (variant % 10 == 7), B transposed',
        "cond": 'variant % 10 == 7 and transB == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-7]', {'variant': 7, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[1-100-130-53-27]', {'variant': 27, 'transB': 1}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-7]', {'variant': 7, 'transB': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_reduce_kernel',
        "lines": [
            'hipLaunchKernelGGL(gemm_split_reduce_kernel, dim3(rblocks), dim3(256), 0, s, ws, C, n, g.s_split, p.splits);',
            'if (rc != 0 || p.splits == 1) return rc;',
            'int splits = variant < 0 ? 0 : variant / 10;',
        ],
        "when": ('more than one K range (variant // 10 > 1, or the automatic split of a long reduction over few '
                 'tiles)'),
        "cond": 'variant // 10 > 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[2-256-256-1813-20]', {'variant': 20}),
            ('tests/test_gemm_split_gpu.py::test_nt_split_reduction_matches_float64[3-256-128-592-52]', {'variant': 52}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_packed', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pa_kernel<256, 128, 16, 2, 4, 4>',
        "lines": [
            'case 0: hipLaunchKernelGGL((gemm_split_pa_kernel<256, 128, 16, 2, 4, 4>), grid, block, 0, s, g); break;',
            'inline int pa_tile(int variant) { return variant == -1 ? 0 : variant; }   // < -1 or >= kNumPaTiles: refused',
            'switch (t) {',
        ],
        "when": 'packed-A tile 0 (or -1)',
        "cond": 'variant == 0',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-256-300-32-0]', {'variant': 0}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[3-100-70-48-0]', {'variant': 0}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-37-1000-72-0]', {'variant': 0}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_packed', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pa_kernel<256, 256, 16, 2, 4, 2>',
        "lines": [
            'case 1: hipLaunchKernelGGL((gemm_split_pa_kernel<256, 256, 16, 2, 4, 2>), grid, block, 0, s, g); break;',
            'inline int pa_tile(int variant) { return variant == -1 ? 0 : variant; }   // < -1 or >= kNumPaTiles: refused',
            'switch (t) {',
        ],
        "when": 'packed-A tile 1',
        "cond": 'variant == 1',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-256-300-32-1]', {'variant': 1}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[3-100-70-48-1]', {'variant': 1}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-37-1000-72-1]', {'variant': 1}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_packed', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pa_kernel<128, 128, 16, 2, 2, 3>',
        "lines": [
            'default: hipLaunchKernelGGL((gemm_split_pa_kernel<128, 128, 16, 2, 2, 3>), grid, block, 0, s, g); break;',
            'inline int pa_tile(int variant) { return variant == -1 ? 0 : variant; }   // < -1 or >= kNumPaTiles: refused',
            'switch (t) {',
        ],
        "when": 'packed-A tile 2',
        "cond": 'variant == 2',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-256-300-32-2]', {'variant': 2}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[3-100-70-48-2]', {'variant': 2}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-37-1000-72-2]', {'variant': 2}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_packed', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_kernel<128, 128, 16, 2, 2, 3, false, true, true>',
        "lines": [
            'hipLaunchKernelGGL((gemm_split_kernel<128, 128, 16, 2, 2, 3, false, true, true>), dim3((unsigned)blocks), dim3(256), 0,',
            'inline int pa_tile(int variant) { return variant == -1 ? 0 : variant; }   // < -1 or >= kNumPaTiles: refused',
            'if (t == 3) {',
        ],
        "when": 'packed-A tile 3: the generic kernel with the packed A staged through registers',
        "cond": 'variant == 3',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-256-300-32-3]', {'variant': 3}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[3-100-70-48-3]', {'variant': 3}),
            ('tests/test_gemm_split_gpu.py::test_packed_a_form_equals_the_generic_kernel[2-37-1000-72-3]', {'variant': 3}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pnn_kernel<256, true>',
        "lines": [
            'if (ktail) hipLaunchKernelGGL((gemm_split_pnn_kernel<256, true>), dim3((unsigned)grid), dim3(512), 0, s, g);',
            'const bool ktail = K % 16 != 0;',
            'const int bn = (variant == 1 || variant >= 6) ? 128 : 256;',
            'if (bn == 256) {',
        ],
        "when": 'every wave stages and multiplies, 256 columns (variant 0, -1), K not a multiple of 16',
        "cond": 'variant == 0 and (K % 16 != 0) == True',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-37-1000-72-0]', {'variant': 0, 'K': 72}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[1-512-260-131-0]', {'variant': 0, 'K': 131}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pnn_kernel<256, false>',
        "lines": [
            'else hipLaunchKernelGGL((gemm_split_pnn_kernel<256, false>), dim3((unsigned)grid), dim3(512), 0, s, g);',
            'const bool ktail = K % 16 != 0;',
            'const int bn = (variant == 1 || variant >= 6) ? 128 : 256;',
            'if (bn == 256) {',
        ],
        "when": 'every wave stages and multiplies, 256 columns (variant 0, -1), K a multiple of 16',
        "cond": 'variant == 0 and (K % 16 != 0) == False',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-256-300-32-0]', {'variant': 0, 'K': 32}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[3-100-70-48-0]', {'variant': 0, 'K': 48}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pnn_kernel<128, true>',
        "lines": [
            'if (ktail) hipLaunchKernelGGL((gemm_split_pnn_kernel<128, true>), dim3((unsigned)grid), dim3(512), 0, s, g);',
            'const bool ktail = K % 16 != 0;',
            'const int bn = (variant == 1 || variant >= 6) ? 128 : 256;',
            'if (bn == 256) {',
        ],
        "when": 'every wave stages and multiplies, 128 columns (variant 1), K not a multiple of 16',
        "cond": 'variant == 1 and (K % 16 != 0) == True',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-37-1000-72-1]', {'variant': 1, 'K': 72}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[1-512-260-131-1]', {'variant': 1, 'K': 131}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_pnn_kernel<128, false>',
        "lines": [
            'else hipLaunchKernelGGL((gemm_split_pnn_kernel<128, false>), dim3((unsigned)grid), dim3(512), 0, s, g);',
            'const bool ktail = K % 16 != 0;',
            'const int bn = (variant == 1 || variant >= 6) ? 128 : 256;',
            'if (bn == 256) {',
        ],
        "when": 'every wave stages and multiplies, 128 columns (variant 1), K a multiple of 16',
        "cond": 'variant == 1 and (K % 16 != 0) == False',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-256-300-32-1]', {'variant': 1, 'K': 32}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[3-100-70-48-1]', {'variant': 1, 'K': 48}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_ws_kernel<256, 128, 3, 3, 2, true>',
        "lines": [
            'if (ktail) hipLaunchKernelGGL((gemm_split_ws_kernel<BM_, 128, RA_, RR_, MINW_, true>), gr, bl, 0, s, g);        \\',
            'const bool ktail = K % 16 != 0;',
            'if (variant >= 13) FPSG_WS(128, 2, 3, 4);',
            'else FPSG_WS(256, 3, 3, 2);',
            'if (variant >= 6) {',
        ],
        "when": 'specialised waves, 256-row tiles (variant 6 or 12), K not a multiple of 16',
        "cond": 'variant in (6, 12) and (K % 16 != 0) == True',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-37-1000-72-6]', {'variant': 6, 'K': 72}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-37-1000-72-12]', {'variant': 12, 'K': 72}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[1-512-260-131-6]', {'variant': 6, 'K': 131}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[1-512-260-131-12]', {'variant': 12, 'K': 131}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_ws_kernel<256, 128, 3, 3, 2, false>',
        "lines": [
            'else hipLaunchKernelGGL((gemm_split_ws_kernel<BM_, 128, RA_, RR_, MINW_, false>), gr, bl, 0, s, g);             \\',
            'const bool ktail = K % 16 != 0;',
            'if (variant >= 13) FPSG_WS(128, 2, 3, 4);',
            'else FPSG_WS(256, 3, 3, 2);',
            'if (variant >= 6) {',
        ],
        "when": 'specialised waves, 256-row tiles (variant 6 or 12), K a multiple of 16',
        "cond": 'variant in (6, 12) and (K % 16 != 0) == False',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-256-300-32-6]', {'variant': 6, 'K': 32}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-256-300-32-12]', {'variant': 12, 'K': 32}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[3-100-72-48-6]', {'variant': 6, 'K': 48}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[3-100-72-48-12]', {'variant': 12, 'K': 48}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_ws_kernel<128, 128, 2, 3, 4, true>',
        "lines": [
            'if (ktail) hipLaunchKernelGGL((gemm_split_ws_kernel<BM_, 128, RA_, RR_, MINW_, true>), gr, bl, 0, s, g);        \\',
            'const bool ktail = K % 16 != 0;',
            'if (variant >= 13) FPSG_WS(128, 2, 3, 4);',
            'else FPSG_WS(256, 3, 3, 2);',
            'if (variant >= 6) {',
        ],
        "when": 'specialised waves, 128-row tiles (variant 13 or 14), K not a multiple of 16',
        "cond": 'variant in (13, 14) and (K % 16 != 0) == True',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-37-1000-72-13]', {'variant': 13, 'K': 72}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-37-1000-72-14]', {'variant': 14, 'K': 72}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[1-512-260-131-13]', {'variant': 13, 'K': 131}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[1-512-260-131-14]', {'variant': 14, 'K': 131}),
        ],
    },
    {
        "entry": 'fpsg_gemm_split_nn_persistent', "file": 'gemm_split.hip',
        "kernel": 'gemm_split_ws_kernel<128, 128, 2, 3, 4, false>',
        "lines": [
            'else hipLaunchKernelGGL((gemm_split_ws_kernel<BM_, 128, RA_, RR_, MINW_, false>), gr, bl, 0, s, g);             \\',
            'const bool ktail = K % 16 != 0;',
            'if (variant >= 13) FPSG_WS(128, 2, 3, 4);',
            'else FPSG_WS(256, 3, 3, 2);',
            'if (variant >= 6) {',
        ],
        "when": 'specialised waves, 128-row tiles (variant 13 or 14), K a multiple of 16',
        "cond": 'variant in (13, 14) and (K % 16 != 0) == False',
        "cases": [
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-256-300-32-13]', {'variant': 13, 'K': 32}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[2-256-300-32-14]', {'variant': 14, 'K': 32}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[3-100-72-48-13]', {'variant': 13, 'K': 48}),
            ('tests/test_gemm_split_gpu.py::test_persistent_form_equals_the_tiled_kernels[3-100-72-48-14]', {'variant': 14, 'K': 48}),
        ],
    },
    {
        "entry": 'fpsg_gemm_f32_nn', "file": 'gemm_split.hip',
        "kernel": 'gemm_f32_ws_kernel<128, 128, 2, 4, true>',
        "lines": [
            'if (K % 16 != 0) hipLaunchKernelGGL((gemm_f32_ws_kernel<128, 128, 2, 4, true>), gr, bl, 0, s, g);',
            'const bool small = variant < 0 || variant >= 2;',
            'if (small) {',
        ],
        "when": '128-row tiles (variant 2 or 3, -1), K not a multiple of 16',
        "cond": 'variant in (2, 3) and (K % 16 != 0) == True',
        "cases": [
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-37-1000-72-2]', {'variant': 2, 'K': 72}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-37-1000-72-3]', {'variant': 3, 'K': 72}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[7-300-36-20-2]', {'variant': 2, 'K': 20}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[7-300-36-20-3]', {'variant': 3, 'K': 20}),
        ],
    },
    {
        "entry": 'fpsg_gemm_f32_nn', "file": 'gemm_split.hip',
        "kernel": 'gemm_f32_ws_kernel<128, 128, 2, 4, false>',
        "lines": [
            'else hipLaunchKernelGGL((gemm_f32_ws_kernel<128, 128, 2, 4, false>), gr, bl, 0, s, g);',
            'const bool small = variant < 0 || variant >= 2;',
            'if (small) {',
        ],
        "when": '128-row tiles (variant 2 or 3, -1), K a multiple of 16',
        "cond": 'variant in (2, 3) and (K % 16 != 0) == False',
        "cases": [
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-256-300-32-2]', {'variant': 2, 'K': 32}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-256-300-32-3]', {'variant': 3, 'K': 32}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[3-100-72-48-2]', {'variant': 2, 'K': 48}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[3-100-72-48-3]', {'variant': 3, 'K': 48}),
        ],
    },
    {
        "entry": 'fpsg_gemm_f32_nn', "file": 'gemm_split.hip',
        "kernel": 'gemm_f32_ws_kernel<256, 128, 4, 2, true>',
        "lines": [
            'if (K % 16 != 0) hipLaunchKernelGGL((gemm_f32_ws_kernel<256, 128, 4, 2, true>), gr, bl, 0, s, g);',
            'const bool small = variant < 0 || variant >= 2;',
            'if (small) {',
        ],
        "when": '256-row tiles (variant 0 or 1), K not a multiple of 16',
        "cond": 'variant in (0, 1) and (K % 16 != 0) == True',
        "cases": [
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-37-1000-72-0]', {'variant': 0, 'K': 72}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-37-1000-72-1]', {'variant': 1, 'K': 72}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[7-300-36-20-0]', {'variant': 0, 'K': 20}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[7-300-36-20-1]', {'variant': 1, 'K': 20}),
        ],
    },
    {
        "entry": 'fpsg_gemm_f32_nn', "file": 'gemm_split.hip',
        "kernel": 'gemm_f32_ws_kernel<256, 128, 4, 2, false>',
        "lines": [
            'else hipLaunchKernelGGL((gemm_f32_ws_kernel<256, 128, 4, 2, false>), gr, bl, 0, s, g);',
            'const bool small = variant < 0 || variant >= 2;',
            'if (small) {',
        ],
        "when": '256-row tiles (variant 0 or 1), K a multiple of 16',
        "cond": 'variant in (0, 1) and (K % 16 != 0) == False',
        "cases": [
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-256-300-32-0]', {'variant': 0, 'K': 32}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[2-256-300-32-1]', {'variant': 1, 'K': 32}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[3-100-72-48-0]', {'variant': 0, 'K': 48}),
            ('tests/test_gemm_f32_gpu.py::test_matches_float64_like_the_library[3-100-72-48-1]', {'variant': 1, 'K': 48}),
        ],
    },
    # ---- bnact.hip -----------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_small_kernel<0, 1>',
        "lines": [
            'if (act == kActRelu) FPSG_SMALL(kActRelu);',
            'const bool small = (long)N * L <= kBnSmallMax;',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L <= 16384, activation relu',
        "cond": 'N * L <= 16384 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape0-relu]', {'N': 4, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape0-relu]', {'N': 4, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape6-relu]', {'N': 5, 'L': 64, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape6-relu]', {'N': 5, 'L': 64, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_small_kernel<0, 2>',
        "lines": [
            'else if (act == kActLeaky) FPSG_SMALL(kActLeaky);',
            'const bool small = (long)N * L <= kBnSmallMax;',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L <= 16384, activation leaky',
        "cond": 'N * L <= 16384 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape5-act5]', {'N': 2, 'L': 4160, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape5-act5]', {'N': 2, 'L': 4160, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_small_kernel<0, 0>',
        "lines": [
            'else FPSG_SMALL(kActNone);',
            'const bool small = (long)N * L <= kBnSmallMax;',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L <= 16384, activation none',
        "cond": 'N * L <= 16384 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape2-None]', {'N': 6, 'L': 2048, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape2-None]', {'N': 6, 'L': 2048, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_small_kernel<1, 1>',
        "lines": [
            'if (act == kActRelu) FPSG_SMALL(kActRelu);',
            'if ((long)N * L <= kBnSmallMax) {',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L <= 16384, activation relu',
        "cond": 'N * L <= 16384 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape0-relu]', {'N': 4, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape0-relu]', {'N': 4, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape6-relu]', {'N': 5, 'L': 64, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape6-relu]', {'N': 5, 'L': 64, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_small_kernel<1, 2>',
        "lines": [
            'else if (act == kActLeaky) FPSG_SMALL(kActLeaky);',
            'if ((long)N * L <= kBnSmallMax) {',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L <= 16384, activation leaky',
        "cond": 'N * L <= 16384 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape5-act5]', {'N': 2, 'L': 4160, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape5-act5]', {'N': 2, 'L': 4160, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_small_kernel<1, 0>',
        "lines": [
            'else FPSG_SMALL(kActNone);',
            'if ((long)N * L <= kBnSmallMax) {',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L <= 16384, activation none',
        "cond": 'N * L <= 16384 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape2-None]', {'N': 6, 'L': 2048, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape2-None]', {'N': 6, 'L': 2048, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<0, 0, false>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, false); else if (act == kActLeaky) FPSG_RED(kActLeaky, false); else FPSG_RED(kActNone, false);',
            'launch_reduce<0>(kActNone, x, nullptr, nullptr, pre_bias, N, C, L, S, 0.0f, ws, s);',
            'if (beyond_cache((size_t)N * C * L * sizeof(float))) {',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'training statistics of a tensor with N * L > 16384 (always without activation)',
        "cond": 'N * L > 16384',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<1, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, false); else if (act == kActLeaky) FPSG_RED(kActLeaky, false); else FPSG_RED(kActNone, false);',
            'launch_reduce<1>(act, x, dy, chan, pre_bias, N, C, L, S, slope, ws, s);',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation relu',
        "cond": 'N * L > 16384 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<0, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, false); else if (act == kActLeaky) FPSG_APP(kActLeaky, false); else FPSG_APP(kActNone, false);',
            'launch_apply<0>(act, x, nullptr, chan, nullptr, pre_bias, N, C, L, slope, y, nullptr, s);',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation relu',
        "cond": 'N * L > 16384 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<1, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, false); else if (act == kActLeaky) FPSG_APP(kActLeaky, false); else FPSG_APP(kActNone, false);',
            '[&](float* dxpart) { launch_apply<1>(act, x, dy, chan, coef, pre_bias, N, C, L, slope, dx, dxpart, s); },',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation relu',
        "cond": 'N * L > 16384 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape8-relu]', {'N': 8, 'L': 12544, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape11-relu]', {'N': 37, 'L': 3136, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<1, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, false); else if (act == kActLeaky) FPSG_RED(kActLeaky, false); else FPSG_RED(kActNone, false);',
            'launch_reduce<1>(act, x, dy, chan, pre_bias, N, C, L, S, slope, ws, s);',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation leaky',
        "cond": 'N * L > 16384 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape10-act10]', {'N': 5, 'L': 8196, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape10-act10]', {'N': 5, 'L': 8196, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<0, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, false); else if (act == kActLeaky) FPSG_APP(kActLeaky, false); else FPSG_APP(kActNone, false);',
            'launch_apply<0>(act, x, nullptr, chan, nullptr, pre_bias, N, C, L, slope, y, nullptr, s);',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation leaky',
        "cond": 'N * L > 16384 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape10-act10]', {'N': 5, 'L': 8196, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape10-act10]', {'N': 5, 'L': 8196, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<1, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, false); else if (act == kActLeaky) FPSG_APP(kActLeaky, false); else FPSG_APP(kActNone, false);',
            '[&](float* dxpart) { launch_apply<1>(act, x, dy, chan, coef, pre_bias, N, C, L, slope, dx, dxpart, s); },',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation leaky',
        "cond": 'N * L > 16384 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape10-act10]', {'N': 5, 'L': 8196, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape10-act10]', {'N': 5, 'L': 8196, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<1, 0, false>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, false); else if (act == kActLeaky) FPSG_RED(kActLeaky, false); else FPSG_RED(kActNone, false);',
            'launch_reduce<1>(act, x, dy, chan, pre_bias, N, C, L, S, slope, ws, s);',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation none',
        "cond": 'N * L > 16384 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<0, 0, false>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, false); else if (act == kActLeaky) FPSG_APP(kActLeaky, false); else FPSG_APP(kActNone, false);',
            'launch_apply<0>(act, x, nullptr, chan, nullptr, pre_bias, N, C, L, slope, y, nullptr, s);',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation none',
        "cond": 'N * L > 16384 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<1, 0, false>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, false); else if (act == kActLeaky) FPSG_APP(kActLeaky, false); else FPSG_APP(kActNone, false);',
            '[&](float* dxpart) { launch_apply<1>(act, x, dy, chan, coef, pre_bias, N, C, L, slope, dx, dxpart, s); },',
            'constexpr int kBnSmallMax = 16384;',
        ],
        "when": 'N * L > 16384, activation none',
        "cond": 'N * L > 16384 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[train-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_matches_torch_modules[eval-shape9-None]', {'N': 24, 'L': 2048, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<0, 1, false> and <0, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, false); else if (act == kActLeaky) FPSG_RED(kActLeaky, false); else FPSG_RED(kActNone, false);',
            'launch_reduce<0>(kActNone, x, nullptr, nullptr, pre_bias, N, C, L, S, 0.0f, ws, s);',
        ],
        "when": 'never: compiled, but not launched',
        "cond": None,
        "cases": [],
        "uncovered": ('unreachable: launch_reduce<0> instantiates every activation, but its only call passes '
                      'kActNone (the statistics pass reads x before any activation), so no argument of any entry '
                      'launches these two'),
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<0, 0, true>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, true); else if (act == kActLeaky) FPSG_RED(kActLeaky, true); else FPSG_RED(kActNone, true);',
            'if (beyond_cache((size_t)N * C * L * sizeof(float))) {',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[leaky-5x9x8196-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[none-24x32x2048-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<1, 1, true>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, true); else if (act == kActLeaky) FPSG_RED(kActLeaky, true); else FPSG_RED(kActNone, true);',
            'if (beyond_cache((size_t)N * C * L * sizeof(float))) {',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-eval]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<1, 2, true>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, true); else if (act == kActLeaky) FPSG_RED(kActLeaky, true); else FPSG_RED(kActNone, true);',
            'if (beyond_cache((size_t)N * C * L * sizeof(float))) {',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[leaky-5x9x8196-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_kernel<1, 0, true>',
        "lines": [
            'if (act == kActRelu) FPSG_RED(kActRelu, true); else if (act == kActLeaky) FPSG_RED(kActLeaky, true); else FPSG_RED(kActNone, true);',
            'if (beyond_cache((size_t)N * C * L * sizeof(float))) {',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[none-24x32x2048-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<0, 1, true>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, true); else if (act == kActLeaky) FPSG_APP(kActLeaky, true); else FPSG_APP(kActNone, true);',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-eval]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<0, 2, true>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, true); else if (act == kActLeaky) FPSG_APP(kActLeaky, true); else FPSG_APP(kActNone, true);',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[leaky-5x9x8196-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_fwd', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<0, 0, true>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, true); else if (act == kActLeaky) FPSG_APP(kActLeaky, true); else FPSG_APP(kActNone, true);',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[none-24x32x2048-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd / fpsg_bn_act_bwd_parts', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<1, 1, true>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, true); else if (act == kActLeaky) FPSG_APP(kActLeaky, true); else FPSG_APP(kActNone, true);',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[relu-37x16x56x56-eval]', None),
            ('tests/test_streaming_forms_gpu.py::test_memory_contract_of_the_streaming_forms[bn_act_bwd_parts-sliced-vec-seg+4]', None),
            ('tests/test_streaming_forms_gpu.py::test_memory_contract_of_the_streaming_forms[bn_act_bwd_parts-sliced-vec-batch3]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd / fpsg_bn_act_bwd_parts', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<1, 2, true>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, true); else if (act == kActLeaky) FPSG_APP(kActLeaky, true); else FPSG_APP(kActNone, true);',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[leaky-5x9x8196-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_memory_contract_of_the_streaming_forms[bn_act_bwd_parts-sliced-vec-leaky]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_bwd / fpsg_bn_act_bwd_parts', "file": 'bnact.hip',
        "kernel": 'bn_apply_kernel<1, 0, true>',
        "lines": [
            'if (act == kActRelu) FPSG_APP(kActRelu, true); else if (act == kActLeaky) FPSG_APP(kActLeaky, true); else FPSG_APP(kActNone, true);',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_reduce_and_apply[none-24x32x2048-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_memory_contract_of_the_streaming_forms[bn_act_bwd_parts-sliced-vec-none]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_fwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_ext_kernel<0, false>',
        "lines": [
            'if (!training) hipLaunchKernelGGL(bn_reduce_ext_kernel<0>, grid, dim3(kBnThreads), 0, s, x, pre_bias, N, C, L, S, ws, ext);',
        ],
        "when": "evaluation: the rows' extremes only",
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape2-act2]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_fwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_ext_kernel<1, false>',
        "lines": [
            'else hipLaunchKernelGGL(bn_reduce_ext_kernel<1>, grid, dim3(kBnThreads), 0, s, x, pre_bias, N, C, L, S, ws, ext);',
        ],
        "when": 'training: statistics and extremes',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape2-act2]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape4-None]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_fwd', "file": 'bnact.hip',
        "kernel": 'bn_reduce_ext_kernel<1, true>',
        "lines": [
            'else if (beyond_cache((size_t)N * C * L * sizeof(float))) hipLaunchKernelGGL((bn_reduce_ext_kernel<1, true>), grid, dim3(kBnThreads), 0, s, x, pre_bias, N, C, L, S, ws, ext);',
        ],
        "when": 'training, N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_max_forward_and_backward[leaky-3x16x4736]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_max_forward_and_backward[relu-6x128x2048]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_fwd', "file": 'bnact.hip',
        "kernel": 'bn_max_out_kernel<1>',
        "lines": [
            'if (act == kActRelu) hipLaunchKernelGGL(bn_max_out_kernel<kActRelu>, og, dim3(256), 0, s, ext, chan, rows, C, segs, slope, out, idx);',
        ],
        "when": 'activation relu',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape3-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape3-relu]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_bwd / fpsg_bn_act_max_bwd_coef', "file": 'bnact.hip',
        "kernel": 'bn_max_bwd_coef_kernel<1>',
        "lines": [
            'if (act == kActRelu) FPSG_MAXB(kActRelu); else if (act == kActLeaky) FPSG_MAXB(kActLeaky); else FPSG_MAXB(kActNone);',
        ],
        "when": 'activation relu',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape3-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape3-relu]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_fwd', "file": 'bnact.hip',
        "kernel": 'bn_max_out_kernel<2>',
        "lines": [
            'else if (act == kActLeaky) hipLaunchKernelGGL(bn_max_out_kernel<kActLeaky>, og, dim3(256), 0, s, ext, chan, rows, C, segs, slope, out, idx);',
        ],
        "when": 'activation leaky',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape2-act2]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape2-act2]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_bwd / fpsg_bn_act_max_bwd_coef', "file": 'bnact.hip',
        "kernel": 'bn_max_bwd_coef_kernel<2>',
        "lines": [
            'if (act == kActRelu) FPSG_MAXB(kActRelu); else if (act == kActLeaky) FPSG_MAXB(kActLeaky); else FPSG_MAXB(kActNone);',
        ],
        "when": 'activation leaky',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape2-act2]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape2-act2]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_fwd', "file": 'bnact.hip',
        "kernel": 'bn_max_out_kernel<0>',
        "lines": [
            'else hipLaunchKernelGGL(bn_max_out_kernel<kActNone>, og, dim3(256), 0, s, ext, chan, rows, C, segs, slope, out, idx);',
        ],
        "when": 'activation none',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape1-None]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape1-None]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape4-None]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape4-None]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_bwd / fpsg_bn_act_max_bwd_coef', "file": 'bnact.hip',
        "kernel": 'bn_max_bwd_coef_kernel<0>',
        "lines": [
            'if (act == kActRelu) FPSG_MAXB(kActRelu); else if (act == kActLeaky) FPSG_MAXB(kActLeaky); else FPSG_MAXB(kActNone);',
        ],
        "when": 'activation none',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape1-None]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape1-None]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape4-None]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape4-None]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_bwd', "file": 'bnact.hip',
        "kernel": 'bn_max_apply_kernel<false>',
        "lines": [
            'hipLaunchKernelGGL(beyond_cache((size_t)N * C * L * sizeof(float)) ? bn_max_apply_kernel<true> : bn_max_apply_kernel<false>,',
        ],
        "when": 'N * C * L floats within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[train-shape0-relu]', None),
            ('tests/test_bnact_gpu.py::test_max_variant_matches_unfused_chain[eval-shape1-None]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_max_bwd', "file": 'bnact.hip',
        "kernel": 'bn_max_apply_kernel<true>',
        "lines": [
            'hipLaunchKernelGGL(beyond_cache((size_t)N * C * L * sizeof(float)) ? bn_max_apply_kernel<true> : bn_max_apply_kernel<false>,',
        ],
        "when": 'N * C * L floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_max_forward_and_backward[leaky-3x16x4736]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_max_forward_and_backward[relu-6x128x2048]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 1, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 2); else if (act == kActLeaky) FPSG_PA(kActLeaky, 2); else FPSG_PA(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation relu',
        "cond": 'W % 4 == 0 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape1]', {'W': 28, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape1]', {'W': 28, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape0]', {'W': 56, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape0]', {'W': 56, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 1, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 2); else if (act == kActLeaky) FPSG_PA(kActLeaky, 2); else FPSG_PA(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation relu',
        "cond": 'W % 4 == 0 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape1]', {'W': 28, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape1]', {'W': 28, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape0]', {'W': 56, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape0]', {'W': 56, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<1, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PR(kActRelu, 2); else if (act == kActLeaky) FPSG_PR(kActLeaky, 2); else FPSG_PR(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation relu',
        "cond": 'W % 4 == 0 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape1]', {'W': 28, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape1]', {'W': 28, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape0]', {'W': 56, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape0]', {'W': 56, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 2, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 2); else if (act == kActLeaky) FPSG_PA(kActLeaky, 2); else FPSG_PA(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation leaky',
        "cond": 'W % 4 == 0 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape0-leaky]', {'W': 28, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape0-leaky]', {'W': 28, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 2, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 2); else if (act == kActLeaky) FPSG_PA(kActLeaky, 2); else FPSG_PA(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation leaky',
        "cond": 'W % 4 == 0 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape0-leaky]', {'W': 28, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape0-leaky]', {'W': 28, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<2, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PR(kActRelu, 2); else if (act == kActLeaky) FPSG_PR(kActLeaky, 2); else FPSG_PR(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation leaky',
        "cond": 'W % 4 == 0 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape0-leaky]', {'W': 28, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape0-leaky]', {'W': 28, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 0, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 2); else if (act == kActLeaky) FPSG_PA(kActLeaky, 2); else FPSG_PA(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation none',
        "cond": 'W % 4 == 0 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape0-none]', {'W': 28, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape0-none]', {'W': 28, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 0, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 2); else if (act == kActLeaky) FPSG_PA(kActLeaky, 2); else FPSG_PA(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation none',
        "cond": 'W % 4 == 0 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape0-none]', {'W': 28, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape0-none]', {'W': 28, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<0, 2, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PR(kActRelu, 2); else if (act == kActLeaky) FPSG_PR(kActLeaky, 2); else FPSG_PR(kActNone, 2);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 == 0, activation none',
        "cond": 'W % 4 == 0 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape0-none]', {'W': 28, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape0-none]', {'W': 28, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 1, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 1); else if (act == kActLeaky) FPSG_PA(kActLeaky, 1); else FPSG_PA(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation relu',
        "cond": 'W % 4 != 0 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape3]', {'W': 30, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape3]', {'W': 30, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape5]', {'W': 6, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape5]', {'W': 6, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 1, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 1); else if (act == kActLeaky) FPSG_PA(kActLeaky, 1); else FPSG_PA(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation relu',
        "cond": 'W % 4 != 0 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape3]', {'W': 30, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape3]', {'W': 30, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape5]', {'W': 6, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape5]', {'W': 6, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<1, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PR(kActRelu, 1); else if (act == kActLeaky) FPSG_PR(kActLeaky, 1); else FPSG_PR(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation relu',
        "cond": 'W % 4 != 0 and act == 1',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape3]', {'W': 30, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape3]', {'W': 30, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[train-shape5]', {'W': 6, 'act': 1}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_matches_unfused_chain[eval-shape5]', {'W': 6, 'act': 1}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 2, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 1); else if (act == kActLeaky) FPSG_PA(kActLeaky, 1); else FPSG_PA(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation leaky',
        "cond": 'W % 4 != 0 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape1-leaky]', {'W': 30, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape1-leaky]', {'W': 30, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 2, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 1); else if (act == kActLeaky) FPSG_PA(kActLeaky, 1); else FPSG_PA(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation leaky',
        "cond": 'W % 4 != 0 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape1-leaky]', {'W': 30, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape1-leaky]', {'W': 30, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<2, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PR(kActRelu, 1); else if (act == kActLeaky) FPSG_PR(kActLeaky, 1); else FPSG_PR(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation leaky',
        "cond": 'W % 4 != 0 and act == 2',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape1-leaky]', {'W': 30, 'act': 2}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape1-leaky]', {'W': 30, 'act': 2}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 0, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 1); else if (act == kActLeaky) FPSG_PA(kActLeaky, 1); else FPSG_PA(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation none',
        "cond": 'W % 4 != 0 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape1-none]', {'W': 30, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape1-none]', {'W': 30, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 0, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PA(kActRelu, 1); else if (act == kActLeaky) FPSG_PA(kActLeaky, 1); else FPSG_PA(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation none',
        "cond": 'W % 4 != 0 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape1-none]', {'W': 30, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape1-none]', {'W': 30, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<0, 1, false>',
        "lines": [
            'if (act == kActRelu) FPSG_PR(kActRelu, 1); else if (act == kActLeaky) FPSG_PR(kActLeaky, 1); else FPSG_PR(kActNone, 1);',
            '} else if ((W & 3) == 0) {',
        ],
        "when": 'W % 4 != 0, activation none',
        "cond": 'W % 4 != 0 and act == 0',
        "cases": [
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[train-shape1-none]', {'W': 30, 'act': 0}),
            ('tests/test_bnact_gpu.py::test_pooled_variant_of_the_other_activations_matches_unfused_chain[eval-shape1-none]', {'W': 30, 'act': 0}),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_fwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<0, 1, 2, true>',
        "lines": [
            'hipLaunchKernelGGL((bn_pool_apply_kernel<MODE, kActRelu, 2, true>), grid, dim3(kBnThreads), 0, s, x, dyp, chan, coef, pb,',
        ],
        "when": 'W % 4 == 0, ReLU, N * C * H * W floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[37x16x28x28-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[37x16x28x28-eval]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[8x64x56x56-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_apply_kernel<2, 1, 2, true>',
        "lines": [
            'hipLaunchKernelGGL((bn_pool_apply_kernel<MODE, kActRelu, 2, true>), grid, dim3(kBnThreads), 0, s, x, dyp, chan, coef, pb,',
        ],
        "when": 'W % 4 == 0, ReLU, N * C * H * W floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[37x16x28x28-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[37x16x28x28-eval]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[8x64x56x56-train]', None),
        ],
    },
    {
        "entry": 'fpsg_bn_act_pool_bwd', "file": 'bnact.hip',
        "kernel": 'bn_pool_reduce_kernel<1, 2, true>',
        "lines": [
            'hipLaunchKernelGGL((bn_pool_reduce_kernel<kActRelu, 2, true>), grid, dim3(kBnThreads), 0, s, x, dyp, chan, pb, N, C, H, W,',
        ],
        "when": 'W % 4 == 0, ReLU, N * C * H * W floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[37x16x28x28-train]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[37x16x28x28-eval]', None),
            ('tests/test_streaming_forms_gpu.py::test_bn_pooled_forward_and_backward[8x64x56x56-train]', None),
        ],
    },
    # ---- winograd_fused.hip --------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_wino_conv_fused', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<false, false, false>',
        "lines": [
            ': (parts ? wino4_fused_c64_kernel<false, true> : wino4_fused_c64_kernel<false, false>));',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'no activation, no statistics, y within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_fused_kernel_matches_three_kernel_form[shape0]', None),
            ('tests/test_winograd_gpu.py::test_fused_kernel_matches_three_kernel_form[shape1]', None),
            ('tests/test_winograd_gpu.py::test_fused_kernel_matches_three_kernel_form[shape4]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused_stats', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<false, true, false>',
        "lines": [
            ': (parts ? wino4_fused_c64_kernel<false, true> : wino4_fused_c64_kernel<false, false>));',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'statistics, no activation, y within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_fused_kernel_delivers_batchnorm_partial_sums[False-shape0]', None),
            ('tests/test_winograd_gpu.py::test_fused_kernel_delivers_batchnorm_partial_sums[False-shape1]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused_act', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<true, false, false>',
        "lines": [
            ': (chan ? (parts ? wino4_fused_c64_kernel<true, true> : wino4_fused_c64_kernel<true, false>)',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'activated input, no statistics, y within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[train-64-64-112-6]', None),
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[eval-64-128-56-6]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused_stats', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<true, true, false>',
        "lines": [
            ': (chan ? (parts ? wino4_fused_c64_kernel<true, true> : wino4_fused_c64_kernel<true, false>)',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'activated input and statistics, y within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_fused_kernel_delivers_batchnorm_partial_sums[True-shape0]', None),
            ('tests/test_winograd_gpu.py::test_fused_kernel_delivers_batchnorm_partial_sums[True-shape1]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<false, false, true>',
        "lines": [
            ': (parts ? wino4_fused_c64_kernel<false, true, true> : wino4_fused_c64_kernel<false, false, true>))',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'no activation, no statistics, y beyond 300 MiB',
        "cond": 'N * K * H * H * 4 > 300 << 20',
        "cases": [
            ('tests/test_winograd_gpu.py::test_full_size_layers_against_the_library_and_linearity[layer0]', {'N': 37, 'K': 64, 'H': 224}),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused_stats', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<false, true, true>',
        "lines": [
            ': (parts ? wino4_fused_c64_kernel<false, true, true> : wino4_fused_c64_kernel<false, false, true>))',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'statistics, no activation, y beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[plain-2x64x128x28x36]', None),
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[plain-1x64x16x4x4]', None),
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[plain-37x64x32x56x56]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused_act', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<true, false, true>',
        "lines": [
            'nt ? (chan ? (parts ? wino4_fused_c64_kernel<true, true, true> : wino4_fused_c64_kernel<true, false, true>)',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'activated input, no statistics, y beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[activated-2x64x128x28x36]', None),
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[activated-1x64x16x4x4]', None),
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[activated-37x64x32x56x56]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_conv_fused_stats', "file": 'winograd_fused.hip',
        "kernel": 'wino4_fused_c64_kernel<true, true, true>',
        "lines": [
            'nt ? (chan ? (parts ? wino4_fused_c64_kernel<true, true, true> : wino4_fused_c64_kernel<true, false, true>)',
            'const bool nt = beyond_cache((size_t)N * K * H * W * sizeof(float));',
        ],
        "when": 'activated input and statistics, y beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[activated-2x64x128x28x36]', None),
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[activated-1x64x16x4x4]', None),
            ('tests/test_streaming_forms_gpu.py::test_fused_winograd_convolution[activated-37x64x32x56x56]', None),
        ],
    },
    # ---- winograd_dw.hip -----------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_wino_dw_fused', "file": 'winograd_dw.hip',
        "kernel": 'wino4_dw_c64_kernel<false>',
        "lines": [
            'const kern_t kern = chan ? wino4_dw_c64_kernel<true> : wino4_dw_c64_kernel<false>;',
        ],
        "when": 'chan == NULL: x as it is',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_fused_weight_gradient_matches_three_kernel_form[False-shape0]', None),
            ('tests/test_winograd_gpu.py::test_fused_weight_gradient_matches_three_kernel_form[False-shape4]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_dw_fused', "file": 'winograd_dw.hip',
        "kernel": 'wino4_dw_c64_kernel<true>',
        "lines": [
            'const kern_t kern = chan ? wino4_dw_c64_kernel<true> : wino4_dw_c64_kernel<false>;',
        ],
        "when": 'chan given: relu(BN(x)) formed on the way in',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_fused_weight_gradient_matches_three_kernel_form[True-shape0]', None),
            ('tests/test_winograd_gpu.py::test_fused_weight_gradient_matches_three_kernel_form[True-shape4]', None),
        ],
    },
    # ---- winograd.hip --------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_wino_input_transform', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<2, false, false, false, false>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_input_kernel<2, false>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape2]', {'m': 2, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape3]', {'m': 2, 'H': 28, 'W': 30}),
        ],
    },
    {
        "entry": 'fpsg_wino_input_transform', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, false, false, true, false>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_input_kernel<4, false, false, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape12]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape13]', {'m': 4, 'H': 18, 'W': 12}),
        ],
    },
    {
        "entry": 'fpsg_wino_input_transform', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, false, false, false, false>',
        "lines": [
            'else hipLaunchKernelGGL((wino_input_kernel<4, false>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * C * Ps * sizeof(float))) hipLaunchKernelGGL((wino_input_kernel<4, false, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape9]', {'m': 4, 'H': 28, 'W': 32}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape11]', {'m': 4, 'H': 28, 'W': 28}),
        ],
    },
    {
        "entry": 'fpsg_wino_input_transform_act', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<2, true, false, false, false>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_input_kernel<2, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, chan, pre_bias);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[train-128-128-10-200]', {'m': 2, 'H': 10, 'W': 10}),
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[eval-128-128-10-200]', {'m': 2, 'H': 10, 'W': 10}),
        ],
    },
    {
        "entry": 'fpsg_wino_input_transform_act', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, true, false, true, false>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_input_kernel<4, true, false, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, chan, pre_bias);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[train-128-256-14-90]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[eval-128-256-14-90]', {'m': 4, 'H': 14, 'W': 14}),
        ],
    },
    {
        "entry": 'fpsg_wino_input_transform_act', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, true, true, false, false>',
        "lines": [
            'else if (beyond_cache((size_t)36 * C * Ps * sizeof(float))) hipLaunchKernelGGL((wino_input_kernel<4, true, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, chan, pre_bias);',
        ],
        "when": 'm = 4, whole tiles, 36 x channels x Ps floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_winograd_activated_input_transform', None),
        ],
    },
    {
        "entry": 'fpsg_wino_input_transform_act', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, true, false, false, false>',
        "lines": [
            'else hipLaunchKernelGGL((wino_input_kernel<4, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, chan, pre_bias);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * C * Ps * sizeof(float))) hipLaunchKernelGGL((wino_input_kernel<4, true, true>), grid, dim3(kWinoThreads), 0, static_cast<hipStream_t>(stream), x, C, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, chan, pre_bias);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[train-128-128-56-6]', {'m': 4, 'H': 56, 'W': 56}),
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[train-256-256-28-24]', {'m': 4, 'H': 28, 'W': 28}),
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[eval-128-128-56-6]', {'m': 4, 'H': 56, 'W': 56}),
            ('tests/test_winograd_gpu.py::test_bn_relu_folded_into_next_conv_equals_two_ops[eval-256-256-28-24]', {'m': 4, 'H': 28, 'W': 28}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<2, false, false, false, false>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_output_kernel<2, false>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, nullptr, nullptr);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape2]', {'m': 2, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape3]', {'m': 2, 'H': 28, 'W': 30}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, false, false, false, true>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_output_kernel<4, false, false, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, nullptr, nullptr);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape12]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape13]', {'m': 4, 'H': 18, 'W': 12}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, false, false, false, false>',
        "lines": [
            'else hipLaunchKernelGGL((wino_output_kernel<4, false>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, nullptr, nullptr);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_output_kernel<4, false, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, nullptr, nullptr);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape9]', {'m': 4, 'H': 28, 'W': 32}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape11]', {'m': 4, 'H': 28, 'W': 28}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<2, true, false, false, false>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_output_kernel<2, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, bias, parts);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[2-shape1]', {'m': 2, 'H': 6, 'W': 10}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[2-shape3]', {'m': 2, 'H': 14, 'W': 14}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, true, false, false, true>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_output_kernel<4, true, false, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, bias, parts);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[4-shape5]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[4-shape6]', {'m': 4, 'H': 18, 'W': 12}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[4-shape7]', {'m': 4, 'H': 6, 'W': 10}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, true, false, true, false>',
        "lines": [
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_output_kernel<4, true, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, bias, parts);',
        ],
        "when": 'm = 4, whole tiles, 36 x channels x Ps floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_winograd_output_transform_with_statistics[37x32x28x28]', None),
            ('tests/test_streaming_forms_gpu.py::test_winograd_output_transform_with_statistics[3x8x12x20]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, true, false, false, false>',
        "lines": [
            'else hipLaunchKernelGGL((wino_output_kernel<4, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, bias, parts);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_output_kernel<4, true, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, bias, parts);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[4-shape0]', {'m': 4, 'H': 12, 'W': 20}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[4-shape2]', {'m': 4, 'H': 28, 'W': 28}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_partial_sums[4-shape4]', {'m': 4, 'H': 112, 'W': 112}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_bwd_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<2, true, true, false, false>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_output_kernel<2, true, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, pre_bias, parts, xpre, chan);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_backward_sums[2-shape1]', {'m': 2, 'H': 50, 'W': 30}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_bwd_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, true, true, false, true>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_output_kernel<4, true, true, false, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, pre_bias, parts, xpre, chan);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_backward_sums[4-shape4]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_backward_sums[4-shape5]', {'m': 4, 'H': 18, 'W': 12}),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_bwd_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, true, true, true, false>',
        "lines": [
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_output_kernel<4, true, true, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, pre_bias, parts, xpre, chan);',
        ],
        "when": 'm = 4, whole tiles, 36 x channels x Ps floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_winograd_output_transform_with_backward_sums[37x32x28x28]', None),
            ('tests/test_streaming_forms_gpu.py::test_winograd_output_transform_with_backward_sums[3x7x8x12]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_output_transform_bwd_stats', "file": 'winograd.hip',
        "kernel": 'wino_output_kernel<4, true, true, false, false>',
        "lines": [
            'else hipLaunchKernelGGL((wino_output_kernel<4, true, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, pre_bias, parts, xpre, chan);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_output_kernel<4, true, true, true>), grid, dim3(kWinoThreads), 0, hs, M, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, y, pre_bias, parts, xpre, chan);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_backward_sums[4-shape0]', {'m': 4, 'H': 56, 'W': 56}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_backward_sums[4-shape2]', {'m': 4, 'H': 28, 'W': 28}),
            ('tests/test_winograd_gpu.py::test_output_transform_delivers_batchnorm_backward_sums[4-shape3]', {'m': 4, 'H': 8, 'W': 12}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_grad_output_kernel<2, false, false>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_grad_output_kernel<2>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, dM);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[2-shape4]', {'m': 2, 'H': 14, 'W': 14}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_grad_output_kernel<4, false, true>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_grad_output_kernel<4, false, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, dM);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape2]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape3]', {'m': 4, 'H': 18, 'W': 12}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_grad_output_kernel<4, true, false>',
        "lines": [
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_grad_output_kernel<4, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, dM);',
        ],
        "when": 'm = 4, whole tiles, 36 x channels x Ps floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_winograd_gradient_transforms[37x40x28x28]', None),
            ('tests/test_streaming_forms_gpu.py::test_winograd_gradient_transforms[1x3x4x4]', None),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_output_transform', "file": 'winograd.hip',
        "kernel": 'wino_grad_output_kernel<4, false, false>',
        "lines": [
            'else hipLaunchKernelGGL((wino_grad_output_kernel<4>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, dM);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_grad_output_kernel<4, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, dM);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape0]', {'m': 4, 'H': 112, 'W': 112}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape1]', {'m': 4, 'H': 28, 'W': 28}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape5]', {'m': 4, 'H': 4, 'W': 4}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_transforms', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<2, false, false, false, true>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL((wino_input_kernel<2, false, false, false, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr, dM);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape2]', {'m': 2, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape3]', {'m': 2, 'H': 28, 'W': 30}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[2-shape4]', {'m': 2, 'H': 14, 'W': 14}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_transforms', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, false, false, true, true>',
        "lines": [
            'else if (ragged(m, H, W)) hipLaunchKernelGGL((wino_input_kernel<4, false, false, true, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr, dM);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
        ],
        "when": 'm = 4, H or W no multiple of 4 (ragged edge tiles)',
        "cond": 'm == 4 and (H | W) & 3 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape12]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape13]', {'m': 4, 'H': 18, 'W': 12}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape2]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape3]', {'m': 4, 'H': 18, 'W': 12}),
        ],
    },
    {
        "entry": 'fpsg_wino_grad_transforms', "file": 'winograd.hip',
        "kernel": 'wino_input_kernel<4, false, false, false, true>',
        "lines": [
            'else hipLaunchKernelGGL((wino_input_kernel<4, false, false, false, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr, dM);',
            'inline bool ragged(int m, int H, int W) { return m == 4 && ((H | W) & 3) != 0; }',
            'else if (beyond_cache((size_t)36 * K * Ps * sizeof(float))) hipLaunchKernelGGL((wino_input_kernel<4, false, true, false, true>), grid, dim3(kWinoThreads), 0, hs, dy, K, H, W, tiles_of(H, m), tiles_of(W, m), P, Ps, V, nullptr, nullptr, dM);',
        ],
        "when": 'm = 4, whole tiles, within 300 MiB',
        "cond": 'm == 4 and (H | W) & 3 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape9]', {'m': 4, 'H': 28, 'W': 32}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape11]', {'m': 4, 'H': 28, 'W': 28}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape0]', {'m': 4, 'H': 112, 'W': 112}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape1]', {'m': 4, 'H': 28, 'W': 28}),
            ('tests/test_winograd_gpu.py::test_both_transforms_of_an_output_gradient_from_one_pass[4-shape5]', {'m': 4, 'H': 4, 'W': 4}),
        ],
    },
    {
        "entry": 'fpsg_wino_filter_transform', "file": 'winograd.hip',
        "kernel": 'wino_filter_kernel<2>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL(wino_filter_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), w, K, C, flip_transpose, U);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape2]', {'m': 2, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape3]', {'m': 2, 'H': 28, 'W': 30}),
        ],
    },
    {
        "entry": 'fpsg_wino_filter_transform', "file": 'winograd.hip',
        "kernel": 'wino_filter_kernel<4>',
        "lines": [
            'else hipLaunchKernelGGL(wino_filter_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), w, K, C, flip_transpose, U);',
        ],
        "when": 'm = 4',
        "cond": 'm == 4',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape12]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape13]', {'m': 4, 'H': 18, 'W': 12}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape9]', {'m': 4, 'H': 28, 'W': 32}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape11]', {'m': 4, 'H': 28, 'W': 28}),
        ],
    },
    {
        "entry": 'fpsg_wino_filter_grad_transform', "file": 'winograd.hip',
        "kernel": 'wino_filter_grad_kernel<2>',
        "lines": [
            'if (m == 2) hipLaunchKernelGGL(wino_filter_grad_kernel<2>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), dU, K, C, dw);',
        ],
        "when": 'm = 2',
        "cond": 'm == 2',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape2]', {'m': 2, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape3]', {'m': 2, 'H': 28, 'W': 30}),
        ],
    },
    {
        "entry": 'fpsg_wino_filter_grad_transform', "file": 'winograd.hip',
        "kernel": 'wino_filter_grad_kernel<4>',
        "lines": [
            'else hipLaunchKernelGGL(wino_filter_grad_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), dU, K, C, dw);',
        ],
        "when": 'm = 4',
        "cond": 'm == 4',
        "cases": [
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape12]', {'m': 4, 'H': 14, 'W': 14}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape13]', {'m': 4, 'H': 18, 'W': 12}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape9]', {'m': 4, 'H': 28, 'W': 32}),
            ('tests/test_winograd_gpu.py::test_forward_and_gradients_match_conv2d[shape11]', {'m': 4, 'H': 28, 'W': 28}),
        ],
    },
    # ---- knn.hip -------------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_stream_kernel<',
        "lines": [
            'if (stream_ok) {',
            'const bool stream_ok = knn_stream_serves(C, k) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 &&',
            '!(flags & FPSG_KNN_FORCE_TILE);',
        ],
        "when": ('at most 128 channels, k <= 24, workspace 16-byte aligned, the tile kernel not forced: the '
                 'streaming kernel'),
        "cond": 'C <= 128 and k <= 24',
        "group": 'streaming or score-tile kernel',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-16-5]', {'C': 3, 'k': 5}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[3-3-1024-24]', {'C': 3, 'k': 24}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-128-200-13]', {'C': 128, 'k': 13}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn.hip',
        "kernel": 'knn_kernel<',
        "lines": [
            'FPSG_REQUIRE(layout == FPSG_KNN_CHANNEL_MAJOR, FPSG_E_LIMIT,',
            'const bool stream_ok = knn_stream_serves(C, k) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 &&',
            '!(flags & FPSG_KNN_FORCE_TILE);',
        ],
        "when": ('otherwise (and FPSG_KNN_FORCE_TILE): the score-tile kernel, whose instantiations are the rows '
                 'above'),
        "cond": 'not (C <= 128 and k <= 24)',
        "group": 'streaming or score-tile kernel',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[3-3-33-33]', {'C': 3, 'k': 33}),
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[1-130-300-16]', {'C': 130, 'k': 16}),
            ('tests/test_dgcnn_gpu.py::test_knn_bit_exact_vs_oracle[1-64-4100-32]', {'C': 64, 'k': 32}),
        ],
    },
    # ---- knn_stream.hip ------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_knn_ex', "file": 'knn_stream.hip',
        "kernel": 'knn_stream_kernel<1>',
        "lines": [
            'case 4: return launch_stream<1>(xk, xx, B, N, k, flags, idx, s);',
            'switch (knn_stream_cpad(C)) {',
        ],
        "when": 'channels padded to 4: C <= 4',
        "cond": 'C <= 4',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-16-5]', {'C': 3}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-4-700-24]', {'C': 4}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-1-257-3]', {'C': 1}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn_stream.hip',
        "kernel": 'knn_stream_kernel<16>',
        "lines": [
            'case 64: return launch_stream<16>(xk, xx, B, N, k, flags, idx, s);',
            'switch (knn_stream_cpad(C)) {',
        ],
        "when": 'channels padded to 64: 4 < C <= 64',
        "cond": '4 < C <= 64',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-64-64-20]', {'C': 64}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-48-257-9]', {'C': 48}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-17-2048-20]', {'C': 17}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn_stream.hip',
        "kernel": 'knn_stream_kernel<32>',
        "lines": [
            'case 128: return launch_stream<32>(xk, xx, B, N, k, flags, idx, s);',
            'switch (knn_stream_cpad(C)) {',
        ],
        "when": 'channels padded to 128: 64 < C <= 128',
        "cond": '64 < C <= 128',
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-128-33-20]', {'C': 128}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-100-777-20]', {'C': 100}),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-80-1040-9]', {'C': 80}),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn_stream.hip',
        "kernel": 'knn_stream_prep_kernel<true>',
        "lines": [
            'if (point_major) hipLaunchKernelGGL(knn_stream_prep_kernel<true>, grid, dim3(256), lds, s, x, C, N, CP, xx, xk);',
        ],
        "when": 'point-major input',
        "cond": None,
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-16-5]', None),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-64-1000-20]', None),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-128-200-13]', None),
        ],
    },
    {
        "entry": 'fpsg_knn_ex', "file": 'knn_stream.hip',
        "kernel": 'knn_stream_prep_kernel<false>',
        "lines": [
            'else hipLaunchKernelGGL(knn_stream_prep_kernel<false>, grid, dim3(256), lds, s, x, C, N, CP, xx, xk);',
        ],
        "when": 'channel-major input',
        "cond": None,
        "cases": [
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-3-16-5]', None),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[1-64-1000-20]', None),
            ('tests/test_dgcnn_gpu.py::test_knn_kernels_and_layouts_agree_with_oracle[2-128-200-13]', None),
        ],
    },
    # ---- chamfer.hip ---------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<1, 16>',
        "lines": [
            'default: return launch_fwd<1, 16>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": "cfg = 0 (also what fpsg_chamfer_fwd picks from the batch's size: cfg < 0)",
        "cond": 'cfg == 0',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[0]', {'cfg': 0}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<2, 16>',
        "lines": [
            'case 1: return launch_fwd<2, 16>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": "cfg = 1 (also what fpsg_chamfer_fwd picks from the batch's size: cfg < 0)",
        "cond": 'cfg == 1',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[1]', {'cfg': 1}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<4, 8>',
        "lines": [
            'case 2: return launch_fwd<4, 8>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": "cfg = 2 (also what fpsg_chamfer_fwd picks from the batch's size: cfg < 0)",
        "cond": 'cfg == 2',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[2]', {'cfg': 2}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<8, 4>',
        "lines": [
            'case 3: return launch_fwd<8, 4>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": "cfg = 3 (also what fpsg_chamfer_fwd picks from the batch's size: cfg < 0)",
        "cond": 'cfg == 3',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[3]', {'cfg': 3}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<4, 4>',
        "lines": [
            'case 4: return launch_fwd<4, 4>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": 'cfg = 4',
        "cond": 'cfg == 4',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[4]', {'cfg': 4}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<2, 8>',
        "lines": [
            'case 5: return launch_fwd<2, 8>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": "cfg = 5 (also what fpsg_chamfer_fwd picks from the batch's size: cfg < 0)",
        "cond": 'cfg == 5',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[5]', {'cfg': 5}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_variant', "file": 'chamfer.hip',
        "kernel": 'chamfer_fwd_kernel<2, 4>',
        "lines": [
            'case 6: return launch_fwd<2, 4>(xyz1, xyz2, B, N, M, dist1, idx1, dist2, idx2, s);',
            'switch (cfg) {',
            'cfg = n_eq < 4.5 ? 0 /*(1,16)*/ : n_eq < 10 ? 1 /*(2,16)*/ : n_eq < 28 ? 5 /*(2,8)*/',
        ],
        "when": 'cfg = 6',
        "cond": 'cfg == 6',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_two_pass_variant_is_bit_exact[6]', {'cfg': 6}),
        ],
    },
    # ---- chamfer_cross.hip ---------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_chamfer_cross', "file": 'chamfer_cross.hip',
        "kernel": 'chamfer_cross_kernel<2>',
        "lines": [
            'case 2: return launch_cross<2>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);',
            'switch (rows_per_lane(N)) {',
            '__host__ __device__ constexpr int rows_per_lane(int n) { return n <= 512 ? 2 : n <= 1024 ? 4 : n <= 2048 ? 8 : 16; }',
        ],
        "when": 'N <= 512',
        "cond": 'N <= 512',
        "cases": [
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[1-1-3-5]', {'N': 1}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[1-1-17-9]', {'N': 1}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[7-7-3-5]', {'N': 7}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[7-7-17-9]', {'N': 7}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[64-64-3-5]', {'N': 64}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[64-64-17-9]', {'N': 64}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[7-1000-3-5]', {'N': 7}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[7-1000-17-9]', {'N': 7}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_cross', "file": 'chamfer_cross.hip',
        "kernel": 'chamfer_cross_kernel<4>',
        "lines": [
            'case 4: return launch_cross<4>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);',
            'switch (rows_per_lane(N)) {',
            '__host__ __device__ constexpr int rows_per_lane(int n) { return n <= 512 ? 2 : n <= 1024 ? 4 : n <= 2048 ? 8 : 16; }',
        ],
        "when": '512 < N <= 1024',
        "cond": '512 < N <= 1024',
        "cases": [
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[1000-1000-3-5]', {'N': 1000}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[1000-1000-17-9]', {'N': 1000}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_cross', "file": 'chamfer_cross.hip',
        "kernel": 'chamfer_cross_kernel<8>',
        "lines": [
            'case 8: return launch_cross<8>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);',
            'switch (rows_per_lane(N)) {',
            '__host__ __device__ constexpr int rows_per_lane(int n) { return n <= 512 ? 2 : n <= 1024 ? 4 : n <= 2048 ? 8 : 16; }',
        ],
        "when": '1024 < N <= 2048',
        "cond": '1024 < N <= 2048',
        "cases": [
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[2047-2047-3-5]', {'N': 2047}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[2047-2047-17-9]', {'N': 2047}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[2048-2048-3-5]', {'N': 2048}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[2048-2048-17-9]', {'N': 2048}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[2048-64-3-5]', {'N': 2048}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[2048-64-17-9]', {'N': 2048}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_cross', "file": 'chamfer_cross.hip',
        "kernel": 'chamfer_cross_kernel<16>',
        "lines": [
            'default: return launch_cross<16>(xyz1, xyz2, Na, Nb, N, M, sym, out, s);',
            'switch (rows_per_lane(N)) {',
            '__host__ __device__ constexpr int rows_per_lane(int n) { return n <= 512 ? 2 : n <= 1024 ? 4 : n <= 2048 ? 8 : 16; }',
        ],
        "when": 'N > 2048',
        "cond": 'N > 2048',
        "cases": [
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[4096-4096-3-5]', {'N': 4096}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[4096-4096-1-1]', {'N': 4096}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[4096-2047-3-5]', {'N': 4096}),
            ('tests/test_chamfer_cross_gpu.py::test_against_float64_brute_force[4096-2047-1-1]', {'N': 4096}),
        ],
    },
    # ---- chamfer_tiled.hip ---------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_tile_kernel<8, 4>',
        "lines": [
            'rc = c.W == 4 ? launch_tiles<8, 4>(xyz1, xyz2, B, N, M, c, row_keys, col_keys, s)',
            'if (c.R == 8) {',
            'R = (variant / 100) ? 8 : 4;',
            'W = (variant / 10) % 10;',
        ],
        "when": '512 rows a workgroup, 4 wave(s) (the automatic choice takes W = 4)',
        "cond": '(8 if variant // 100 else 4) == 8 and variant // 10 % 10 == 4',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-141]', {'variant': 141}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-141]', {'variant': 141}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-144]', {'variant': 144}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-144]', {'variant': 144}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-148]', {'variant': 148}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-148]', {'variant': 148}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_tile_kernel<8, 2>',
        "lines": [
            ': c.W == 2 ? launch_tiles<8, 2>(xyz1, xyz2, B, N, M, c, row_keys, col_keys, s)',
            'if (c.R == 8) {',
            'R = (variant / 100) ? 8 : 4;',
            'W = (variant / 10) % 10;',
        ],
        "when": '512 rows a workgroup, 2 wave(s)',
        "cond": '(8 if variant // 100 else 4) == 8 and variant // 10 % 10 == 2',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-121]', {'variant': 121}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-121]', {'variant': 121}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-122]', {'variant': 122}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-122]', {'variant': 122}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_tile_kernel<8, 1>',
        "lines": [
            ': launch_tiles<8, 1>(xyz1, xyz2, B, N, M, c, row_keys, col_keys, s);',
            'if (c.R == 8) {',
            'R = (variant / 100) ? 8 : 4;',
            'W = (variant / 10) % 10;',
        ],
        "when": '512 rows a workgroup, 1 wave(s)',
        "cond": '(8 if variant // 100 else 4) == 8 and variant // 10 % 10 == 1',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-111]', {'variant': 111}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-111]', {'variant': 111}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_tile_kernel<4, 4>',
        "lines": [
            'rc = c.W == 4 ? launch_tiles<4, 4>(xyz1, xyz2, B, N, M, c, row_keys, col_keys, s)',
            'if (c.R == 8) {',
            'R = (variant / 100) ? 8 : 4;',
            'W = (variant / 10) % 10;',
        ],
        "when": '256 rows a workgroup, 4 wave(s) (the automatic choice takes W = 4)',
        "cond": '(8 if variant // 100 else 4) == 4 and variant // 10 % 10 == 4',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-41]', {'variant': 41}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-41]', {'variant': 41}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-44]', {'variant': 44}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-44]', {'variant': 44}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-49]', {'variant': 49}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-49]', {'variant': 49}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_tile_kernel<4, 2>',
        "lines": [
            ': c.W == 2 ? launch_tiles<4, 2>(xyz1, xyz2, B, N, M, c, row_keys, col_keys, s)',
            'if (c.R == 8) {',
            'R = (variant / 100) ? 8 : 4;',
            'W = (variant / 10) % 10;',
        ],
        "when": '256 rows a workgroup, 2 wave(s)',
        "cond": '(8 if variant // 100 else 4) == 4 and variant // 10 % 10 == 2',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-21]', {'variant': 21}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-21]', {'variant': 21}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_tile_kernel<4, 1>',
        "lines": [
            ': launch_tiles<4, 1>(xyz1, xyz2, B, N, M, c, row_keys, col_keys, s);',
            'if (c.R == 8) {',
            'R = (variant / 100) ? 8 : 4;',
            'W = (variant / 10) % 10;',
        ],
        "when": '256 rows a workgroup, 1 wave(s)',
        "cond": '(8 if variant // 100 else 4) == 4 and variant // 10 % 10 == 1',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-11]', {'variant': 11}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-11]', {'variant': 11}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-14]', {'variant': 14}),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[2-129-4096-14]', {'variant': 14}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled_losses', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_finalize_kernel<true>',
        "lines": [
            'hipLaunchKernelGGL(chamfer_finalize_kernel<true>, grid, dim3(kFinThreads), 0, s, xyz1, xyz2, N, M, c.RT, c.CS, c.R,',
            'if (loss)',
        ],
        "when": "the entry with the episode's loss sums",
        "cond": None,
        "cases": [
            ('tests/test_chamfer_gpu.py::test_episode_losses_equal_the_separate_operations[7-301-258-3]', None),
            ('tests/test_chamfer_gpu.py::test_episode_losses_equal_the_separate_operations[37-2048-2048-5]', None),
            ('tests/test_chamfer_gpu.py::test_episode_losses_equal_the_separate_operations[9-4096-3000-9]', None),
        ],
    },
    {
        "entry": 'fpsg_chamfer_fwd_tiled', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_finalize_kernel<false>',
        "lines": [
            'hipLaunchKernelGGL(chamfer_finalize_kernel<false>, grid, dim3(kFinThreads), 0, s, xyz1, xyz2, N, M, c.RT, c.CS, c.R,',
            'if (loss)',
        ],
        "when": 'the entry without loss sums',
        "cond": None,
        "cases": [
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[3-1000-777-141]', None),
            ('tests/test_chamfer_gpu.py::test_every_tiled_variant_is_bit_exact[1-4096-3000-41]', None),
        ],
    },
    {
        "entry": 'fpsg_chamfer_bwd_sorted', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_bwd_sorted_kernel<true, false>',
        "lines": [
            'if (NBP == 2048) { if (pair) FPSG_BWD_LAUNCH(true, true); else FPSG_BWD_LAUNCH(true, false); }',
            'const int NBP = nmax <= 2048 ? 2048 : 4096;',
        ],
        "when": 'max(N, M) <= 2048, per-point gradients given',
        "cond": 'max(N, M) <= 2048',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_bwd_bit_exact_vs_oracle[3-333-1000-fpsg_chamfer_bwd_sorted]', {'N': 333, 'M': 1000}),
            ('tests/test_chamfer_gpu.py::test_bwd_bit_exact_vs_oracle[5-2048-2048-fpsg_chamfer_bwd_sorted]', {'N': 2048, 'M': 2048}),
            ('tests/test_chamfer_gpu.py::test_bwd_bit_exact_vs_oracle[2-1-50-fpsg_chamfer_bwd_sorted]', {'N': 1, 'M': 50}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_bwd_sorted', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_bwd_sorted_kernel<false, false>',
        "lines": [
            'else             { if (pair) FPSG_BWD_LAUNCH(false, true); else FPSG_BWD_LAUNCH(false, false); }',
            'const int NBP = nmax <= 2048 ? 2048 : 4096;',
        ],
        "when": 'max(N, M) > 2048, per-point gradients given',
        "cond": 'max(N, M) > 2048',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_bwd_bit_exact_vs_oracle[2-4096-3000-fpsg_chamfer_bwd_sorted]', {'N': 4096, 'M': 3000}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_bwd_losses', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_bwd_sorted_kernel<true, true>',
        "lines": [
            'if (NBP == 2048) { if (pair) FPSG_BWD_LAUNCH(true, true); else FPSG_BWD_LAUNCH(true, false); }',
            'const int NBP = nmax <= 2048 ? 2048 : 4096;',
        ],
        "when": 'max(N, M) <= 2048, the gradient a constant per cloud pair',
        "cond": 'max(N, M) <= 2048',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_episode_losses_equal_the_separate_operations[7-301-258-3]', {'N': 301, 'M': 258}),
            ('tests/test_chamfer_gpu.py::test_episode_losses_equal_the_separate_operations[37-2048-2048-5]', {'N': 2048, 'M': 2048}),
        ],
    },
    {
        "entry": 'fpsg_chamfer_bwd_losses', "file": 'chamfer_tiled.hip',
        "kernel": 'chamfer_bwd_sorted_kernel<false, true>',
        "lines": [
            'else             { if (pair) FPSG_BWD_LAUNCH(false, true); else FPSG_BWD_LAUNCH(false, false); }',
            'const int NBP = nmax <= 2048 ? 2048 : 4096;',
        ],
        "when": 'max(N, M) > 2048, the gradient a constant per cloud pair',
        "cond": 'max(N, M) > 2048',
        "cases": [
            ('tests/test_chamfer_gpu.py::test_episode_losses_equal_the_separate_operations[9-4096-3000-9]', {'N': 4096, 'M': 3000}),
        ],
    },
    # ---- emd.hip -------------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<0, false, 4>',
        "lines": [
            'rc = own4 ? sweep<kRatioL, false, 4>(a, B, s, "fpsg_emd_approx(ratioL)")',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kRatioL: forward only, four owners a wave (variant bit 1)',
        "cond": 'variant in (2, 3)',
        "group": 'emd kRatioL',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-3]', {'variant': 3}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<0, false, 2>',
        "lines": [
            ': sweep<kRatioL, false>(a, B, s, "fpsg_emd_approx(ratioL)");',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kRatioL: two owners a wave (and every call with gradients)',
        "cond": 'variant in (0, 1)',
        "group": 'emd kRatioL',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[3-100-300]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[2-101-67]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[1-3-258]', None),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<1, false, 4>',
        "lines": [
            'rc = own4 ? sweep<kRatioR, false, 4>(a, B, s, "fpsg_emd_approx(ratioR)")',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kRatioR: forward only, four owners a wave (variant bit 1)',
        "cond": 'variant in (2, 3)',
        "group": 'emd kRatioR',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-3]', {'variant': 3}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<1, false, 2>',
        "lines": [
            ': sweep<kRatioR, false>(a, B, s, "fpsg_emd_approx(ratioR)");',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kRatioR: two owners a wave (and every call with gradients)',
        "cond": 'variant in (0, 1)',
        "group": 'emd kRatioR',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[3-100-300]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[2-101-67]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[1-3-258]', None),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<2, false, 4>',
        "lines": [
            'rc = own4 ? sweep<kMatch, false, 4>(a, B, s, "fpsg_emd_approx(match)")',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kMatch: forward only, four owners a wave (variant bit 1), separate sweeps',
        "cond": 'variant in (2,)',
        "group": 'emd kMatch',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-2]', {'variant': 2}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-2]', {'variant': 2}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<2, false, 2>',
        "lines": [
            ': sweep<kMatch, false>(a, B, s, "fpsg_emd_approx(match)");',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kMatch: two owners a wave, separate sweeps',
        "cond": 'variant in (0,)',
        "group": 'emd kMatch',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-0]', {'variant': 0}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-0]', {'variant': 0}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<4, false, 4>',
        "lines": [
            'rc = own4 ? sweep<kMatchRatioQ, false, 4>(a, B, s, "fpsg_emd_approx(match+ratioL)")',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kMatchRatioQ: forward only, four owners a wave (variant bit 1), merged sweeps (variant bit 0)',
        "cond": 'variant in (3,)',
        "group": 'emd kMatchRatioQ',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-3]', {'variant': 3}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<4, false, 2>',
        "lines": [
            ': sweep<kMatchRatioQ, false>(a, B, s, "fpsg_emd_approx(match+ratioL)");',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kMatchRatioQ: two owners a wave, merged sweeps (variant bit 0)',
        "cond": 'variant in (1,)',
        "group": 'emd kMatchRatioQ',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-1]', {'variant': 1}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<5, false, 4>',
        "lines": [
            'rc = own4 ? sweep<kMatchRatioZ, false, 4>(a, B, s, "fpsg_emd_approx(match+ratioL)")',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kMatchRatioZ: forward only, four owners a wave (variant bit 1), merged sweeps (variant bit 0)',
        "cond": 'variant in (3,)',
        "group": 'emd kMatchRatioZ',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-3]', {'variant': 3}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-3]', {'variant': 3}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<5, false, 2>',
        "lines": [
            ': sweep<kMatchRatioZ, false>(a, B, s, "fpsg_emd_approx(match+ratioL)");',
            'const bool merged = forward_only && (variant & 1);',
            'const bool own4 = forward_only && (variant & 2);',
            'if (variant < 0) variant = ((long)N * M >= 256L * 256L ? 1 : 0) | ((long)B * (N > M ? N : M) >= 32768 ? 2 : 0);',
        ],
        "when": 'kMatchRatioZ: two owners a wave, merged sweeps (variant bit 0)',
        "cond": 'variant in (1,)',
        "group": 'emd kMatchRatioZ',
        "cases": [
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[3-100-300-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[2-512-512-1]', {'variant': 1}),
            ('tests/test_emd_gpu.py::test_forward_only_variants_vs_oracle[1-3-258-1]', {'variant': 1}),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<2, true, 2>',
        "lines": [
            'rc = sweep<kMatch, true>(a, B, s, "fpsg_emd_approx(match+grad)");',
            '} else if (gxyz1) {',
        ],
        "when": 'gxyz1 given: the assignment sweep with the gradient',
        "cond": None,
        "cases": [
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[3-100-300]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[2-101-67]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[1-3-258]', None),
        ],
    },
    {
        "entry": 'fpsg_emd_approx_variant', "file": 'emd.hip',
        "kernel": 'emd_sweep_kernel<3, true, 2>',
        "lines": [
            'if ((rc = sweep<kGradOther, true>(a, B, s, "fpsg_emd_approx(grad2)"))) return rc;',
            'if (gxyz2) {  // same weights seen from cloud 2',
        ],
        "when": 'gxyz2 given: the gradient seen from cloud 2',
        "cond": None,
        "cases": [
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[3-100-300]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[2-101-67]', None),
            ('tests/test_emd_gpu.py::test_cost_and_grads_vs_oracle[1-3-258]', None),
        ],
    },
    # ---- adam.hip ------------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_adam_step_ema', "file": 'adam.hip',
        "kernel": 'adam_kernel<float const*, true, float*, float>',
        "lines": [
            'return launch_adam<const float*, true>("fpsg_adam_step_ema", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,',
            'if (grad_scale_dev)',
        ],
        "when": 'grad_scale_dev given: the scale read on the device',
        "cond": None,
        "cases": [
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[1025_0]', None),
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[3074]', None),
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[3]', None),
        ],
    },
    {
        "entry": 'fpsg_adam_step_ema', "file": 'adam.hip',
        "kernel": 'adam_kernel<float, true, float*, float>',
        "lines": [
            'return launch_adam<float, true>("fpsg_adam_step_ema", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step,',
            'if (grad_scale_dev)',
        ],
        "when": "grad_scale_dev == NULL: the host's scale",
        "cond": None,
        "cases": [
            ('tests/test_ema_gpu.py::test_shadow_follows_the_float64_recurrence[0.9-flat]', None),
            ('tests/test_ema_gpu.py::test_shadow_follows_the_float64_recurrence[0.9999-flat]', None),
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[1025_0]', None),
        ],
    },
    {
        "entry": 'fpsg_adam_step_segments_ema', "file": 'adam.hip',
        "kernel": 'adam_ptr_kernel<float const*, true, float*, float>',
        "lines": [
            'return launch_adam_segments<const float*, true>("fpsg_adam_step_segments_ema", param, grad_ptrs, seg_off, nseg, exp_avg,',
            'if (grad_scale_dev)',
        ],
        "when": 'grad_scale_dev given: the scale read on the device',
        "cond": None,
        "cases": [
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[1025_1]', None),
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[3074]', None),
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[3]', None),
        ],
    },
    {
        "entry": 'fpsg_adam_step_segments_ema', "file": 'adam.hip',
        "kernel": 'adam_ptr_kernel<float, true, float*, float>',
        "lines": [
            'return launch_adam_segments<float, true>("fpsg_adam_step_segments_ema", param, grad_ptrs, seg_off, nseg, exp_avg,',
            'if (grad_scale_dev)',
        ],
        "when": "grad_scale_dev == NULL: the host's scale",
        "cond": None,
        "cases": [
            ('tests/test_ema_gpu.py::test_shadow_follows_the_float64_recurrence[0.9-segments]', None),
            ('tests/test_ema_gpu.py::test_shadow_follows_the_float64_recurrence[0.9999-segments]', None),
            ('tests/test_ema_gpu.py::test_parameters_and_moments_equal_the_existing_entries_bit_for_bit[1025_1]', None),
        ],
    },
    # ---- conv_first.hip ------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_conv_first_dw_fold', "file": 'conv_first.hip',
        "kernel": 'conv_first_dw_kernel<112, true>',
        "lines": [
            'hipLaunchKernelGGL((conv_first_dw_kernel<112, true>), dim3(blocks), dim3(kFirstThreads), 0, s, x, dy, fa, H, W, segs_per_row, n_segs, ws);',
            'const int px = W % 112 == 0 ? 112 : 64;',
            'const bool fold = fa.y != nullptr;',
            'if (px == 112 && fold)',
        ],
        "when": 'W a multiple of 112, the BatchNorm backward folded in',
        "cond": 'W % 112 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient_with_the_batchnorm_backward_folded_in[shape0]', {'W': 224}),
        ],
    },
    {
        "entry": 'fpsg_conv_first_dw', "file": 'conv_first.hip',
        "kernel": 'conv_first_dw_kernel<112, false>',
        "lines": [
            'hipLaunchKernelGGL((conv_first_dw_kernel<112, false>), dim3(blocks), dim3(kFirstThreads), 0, s, x, dy, fa, H, W, segs_per_row, n_segs, ws);',
            'const int px = W % 112 == 0 ? 112 : 64;',
            'const bool fold = fa.y != nullptr;',
            'else if (px == 112)',
        ],
        "when": 'W a multiple of 112',
        "cond": 'W % 112 == 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient[shape3]', {'W': 224}),
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient[shape5]', {'W': 112}),
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient[shape6]', {'W': 336}),
        ],
    },
    {
        "entry": 'fpsg_conv_first_dw_fold', "file": 'conv_first.hip',
        "kernel": 'conv_first_dw_kernel<64, true>',
        "lines": [
            'hipLaunchKernelGGL((conv_first_dw_kernel<64, true>), dim3(blocks), dim3(kFirstThreads), 0, s, x, dy, fa, H, W, segs_per_row, n_segs, ws);',
            'const int px = W % 112 == 0 ? 112 : 64;',
            'const bool fold = fa.y != nullptr;',
            'else if (fold)',
        ],
        "when": 'W no multiple of 112, the BatchNorm backward folded in',
        "cond": 'W % 112 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient_with_the_batchnorm_backward_folded_in[shape1]', {'W': 128}),
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient_with_the_batchnorm_backward_folded_in[shape2]', {'W': 136}),
        ],
    },
    {
        "entry": 'fpsg_conv_first_dw', "file": 'conv_first.hip',
        "kernel": 'conv_first_dw_kernel<64, false>',
        "lines": [
            'hipLaunchKernelGGL((conv_first_dw_kernel<64, false>), dim3(blocks), dim3(kFirstThreads), 0, s, x, dy, fa, H, W, segs_per_row, n_segs, ws);',
            'const int px = W % 112 == 0 ? 112 : 64;',
            'const bool fold = fa.y != nullptr;',
        ],
        "when": 'W no multiple of 112',
        "cond": 'W % 112 != 0',
        "cases": [
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient[shape0]', {'W': 8}),
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient[shape1]', {'W': 36}),
            ('tests/test_winograd_gpu.py::test_first_layer_weight_gradient[shape4]', {'W': 100}),
        ],
    },
    {
        "entry": 'fpsg_conv_first_fwd', "file": 'conv_first.hip',
        "kernel": 'conv_first_fwd_kernel<true, false>',
        "lines": [
            'hipLaunchKernelGGL(conv_first_fwd_kernel<true>, dim3((unsigned)blocks), dim3(kFirstThreads), 0, s, x, w, H, W, Q, y, bias, parts);',
            'else if (parts)',
            'const bool nt = beyond_cache((size_t)N * 64 * H * W * sizeof(float));      // y: 475 MB at 37 images, written once',
        ],
        "when": 'parts given: the BatchNorm partial sums from the epilogue; y within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_first_layer_forward_and_its_batchnorm_partial_sums[shape1]', None),
            ('tests/test_winograd_gpu.py::test_first_layer_forward_and_its_batchnorm_partial_sums[shape3]', None),
            ('tests/test_winograd_gpu.py::test_first_layer_forward_and_its_batchnorm_partial_sums[shape5]', None),
        ],
    },
    {
        "entry": 'fpsg_conv_first_fwd', "file": 'conv_first.hip',
        "kernel": 'conv_first_fwd_kernel<false, false>',
        "lines": [
            'hipLaunchKernelGGL(conv_first_fwd_kernel<false>, dim3((unsigned)blocks), dim3(kFirstThreads), 0, s, x, w, H, W, Q, y, nullptr, nullptr);',
            'const bool nt = beyond_cache((size_t)N * 64 * H * W * sizeof(float));      // y: 475 MB at 37 images, written once',
        ],
        "when": 'no parts; y within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_winograd_gpu.py::test_first_layer_forward_and_its_batchnorm_partial_sums[shape1]', None),
            ('tests/test_winograd_gpu.py::test_first_layer_forward_and_its_batchnorm_partial_sums[shape3]', None),
            ('tests/test_winograd_gpu.py::test_first_layer_forward_and_its_batchnorm_partial_sums[shape5]', None),
        ],
    },
    {
        "entry": 'fpsg_conv_first_fwd', "file": 'conv_first.hip',
        "kernel": 'conv_first_fwd_kernel<true, true>',
        "lines": [
            'hipLaunchKernelGGL((conv_first_fwd_kernel<true, true>), dim3((unsigned)blocks), dim3(kFirstThreads), 0, s, x, w, H, W, Q, y, bias, parts);',
            'if (parts && nt)',
            'const bool nt = beyond_cache((size_t)N * 64 * H * W * sizeof(float));      // y: 475 MB at 37 images, written once',
        ],
        "when": 'parts given; y beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_first_layer_forward[3x30x36]', None),
            ('tests/test_streaming_forms_gpu.py::test_first_layer_forward[37x56x100]', None),
        ],
    },
    {
        "entry": 'fpsg_conv_first_fwd', "file": 'conv_first.hip',
        "kernel": 'conv_first_fwd_kernel<false, true>',
        "lines": [
            'hipLaunchKernelGGL((conv_first_fwd_kernel<false, true>), dim3((unsigned)blocks), dim3(kFirstThreads), 0, s, x, w, H, W, Q, y, nullptr, nullptr);',
            'else if (nt)',
            'const bool nt = beyond_cache((size_t)N * 64 * H * W * sizeof(float));      // y: 475 MB at 37 images, written once',
        ],
        "when": 'no parts; y beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_first_layer_forward[3x30x36]', None),
            ('tests/test_streaming_forms_gpu.py::test_first_layer_forward[37x56x100]', None),
        ],
    },
    # ---- decoder.hip ---------------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_dec1_fwd_ld', "file": 'decoder.hip',
        "kernel": 'dec1_fwd_kernel<false>',
        "lines": [
            'auto kern = beyond_cache((size_t)G * D * B * P * sizeof(float)) ? dec1_fwd_kernel<true> : dec1_fwd_kernel<false>;',
        ],
        "when": 'G * D * B * P floats within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_dec1_gpu.py::test_k9_against_float64[g2d70b7p32-train-0]', None),
            ('tests/test_dec1_gpu.py::test_k9_against_float64[g1d33b3p128-eval-1]', None),
            ('tests/test_dec1_gpu.py::test_k9_against_float64[g2d40b130p4-train-1]', None),
        ],
    },
    {
        "entry": 'fpsg_dec1_fwd_ld', "file": 'decoder.hip',
        "kernel": 'dec1_fwd_kernel<true>',
        "lines": [
            'auto kern = beyond_cache((size_t)G * D * B * P * sizeof(float)) ? dec1_fwd_kernel<true> : dec1_fwd_kernel<false>;',
        ],
        "when": 'G * D * B * P floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g2d70b7p32-train-0]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g1d33b3p128-eval-1]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g2d40b130p4-train-1]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g1d96b16p128-train-2]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g2d70b7p32-train-accumulate-0]', None),
        ],
    },
    {
        "entry": 'fpsg_dec1_bwd_ld', "file": 'decoder.hip',
        "kernel": 'dec1_bwd_kernel<false>',
        "lines": [
            'auto kern = beyond_cache((size_t)G * D * B * P * sizeof(float)) ? dec1_bwd_kernel<true> : dec1_bwd_kernel<false>;',
        ],
        "when": 'G * D * B * P floats within 300 MiB',
        "cond": None,
        "cases": [
            ('tests/test_dec1_gpu.py::test_k9_against_float64[g2d70b7p32-train-0]', None),
            ('tests/test_dec1_gpu.py::test_k9_against_float64[g1d33b3p128-eval-1]', None),
            ('tests/test_dec1_gpu.py::test_k9_against_float64[g2d40b130p4-train-1]', None),
        ],
    },
    {
        "entry": 'fpsg_dec1_bwd_ld', "file": 'decoder.hip',
        "kernel": 'dec1_bwd_kernel<true>',
        "lines": [
            'auto kern = beyond_cache((size_t)G * D * B * P * sizeof(float)) ? dec1_bwd_kernel<true> : dec1_bwd_kernel<false>;',
        ],
        "when": 'G * D * B * P floats beyond 300 MiB; reached at small shapes in the zero-threshold build of the tests (build/libfpsg_hip_stream.so)',
        "cond": None,
        "cases": [
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g2d70b7p32-train-0]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g1d33b3p128-eval-1]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g2d40b130p4-train-1]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g1d96b16p128-train-2]', None),
            ('tests/test_streaming_forms_gpu.py::test_decoder_first_layer[g2d70b7p32-train-accumulate-0]', None),
        ],
    },
    # ---- mesh_sample.hip -----------------------------------------------------------------------------------------
    {
        "entry": 'fpsg_mesh_cdf', "file": 'mesh_sample.hip',
        "kernel": 'mesh_scan_block_kernel',
        "lines": [
            'hipLaunchKernelGGL(mesh_scan_block_kernel, dim3((unsigned)nb), dim3(kScanT), 0, st, area, F, amax,',
            'constexpr int kScanP = 4;                // faces per thread',
            'constexpr int kScanT = 256;              // threads of a scan workgroup',
        ],
        "when": 'at most 1024 faces: one scan workgroup',
        "cond": 'F <= 1024',
        "cases": [
            ('tests/test_meshes_gpu.py::test_sampling_equals_the_restatement_bit_for_bit[1-1]', {'F': 1}),
            ('tests/test_meshes_gpu.py::test_sampling_equals_the_restatement_bit_for_bit[777-333]', {'F': 777}),
            ('tests/test_meshes_gpu.py::test_sampling_equals_the_restatement_bit_for_bit[65-4096]', {'F': 65}),
        ],
    },
    {
        "entry": 'fpsg_mesh_cdf', "file": 'mesh_sample.hip',
        "kernel": 'mesh_scan_sums_kernel',
        "lines": [
            'if (nb > 1) {',
            'hipLaunchKernelGGL(mesh_scan_sums_kernel, dim3(1), dim3(kScanT), 0, st, sums, nb);',
            'hipLaunchKernelGGL(mesh_scan_add_kernel, dim3((unsigned)nb), dim3(kScanT), 0, st, reinterpret_cast<u64*>(cdf), F,',
            'constexpr int kScanP = 4;                // faces per thread',
        ],
        "when": 'more than 1024 faces: the second scan level',
        "cond": 'F > 1024',
        "cases": [
            ('tests/test_meshes_gpu.py::test_sampling_equals_the_restatement_bit_for_bit[20480-2048]', {'F': 20480}),
        ],
    },
]

# ---- sources whose entries each launch one fixed sequence of kernels, whatever the sizes ------------------------------------
FILES_WITHOUT_A_CHOICE = {
    "capi.hip": "no kernel",
    "dcd.hip": "one kernel",
    "dist_profile.hip": "one kernel",
    "edge.hip": "forward; backward centre + scatter",
    "emd_exact.hip": "one kernel",
    "maxbwd.hip": "gather; sort + scatter; prep; dw -- one entry each, plain kernels",
    "mesh_normals.hip": "one kernel",
    "mesh_render.hip": "project, raster, large-face raster, shade: the shade kernel's mode (flat, smooth, materials) is "
                       "fixed by the entry, not chosen from its arguments",
    "occupancy.hip": "one kernel",
    "point_mesh.hip": "chunk + finish",
}

