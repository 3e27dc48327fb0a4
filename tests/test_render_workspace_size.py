"""nerfart_volsdf_render_workspace_bytes against the layout carve_render carves (csrc/volsdf_render.hip), buffer by buffer, and monotone in the ray
count.  The segment-ordered final stage takes its buffers - the h7 rows of a whole chunk's segment launch included - out of the sampler's region,
which is dead by then: the size is the sum of the buffers listed here and nothing else.  Host arithmetic only."""
import pytest


def _total(sizes):
    return sum((b + 255) // 256 * 256 for b in sizes)


def _sampler(R, n_init, n_up, n_final, max_iter):
    cap = n_init + max_iter * n_up
    return _total([4 * R * cap] * 4 + [4 * R * n_up] * 2 + [4 * R]            # dA, sA, dB, sB, d_new, s_new, beta_plus
                  + [4 * R] * 2 + [4 * 64]                                    # act0, act1, count
                  + [4 * n_init, 4 * (n_up + 2), 4 * n_final]                 # t_init, u_up, u_final
                  + [4 * R] + [12 * R] * 2 + [4 * R] * 2                      # esc_list, c_o, c_dn, c_near, c_far
                  + [4 * R * n_final] * 2 + [4 * R] * 2)                      # c_u, c_d_fine, c_beta, c_iter


def _render(R, ns, ni, max_iter, k3):
    P, rk = ns + ni, min(k3, R)
    return _total([12 * R, 4 * R * ni, 4 * R * ns, 4 * ns]                    # rays_dn, d_fine, d_coarse, t_coarse
                  + [4 * R * P] * 2 + [12 * R * P] * 2 + [4 * R] * 2          # d_all, sdf, nabla, rad, beta_map, iter_usage
                  + [4 * rk * P * 256]                                        # h7 of one chunk of the plain loop
                  + [_sampler(R, 4 * ns, 4 * ns, ni, max_iter), 256 << 20])   # the sampler's region, grad(SDF) scratch


@pytest.mark.parametrize("R,k3", [(1, 1), (300, 32), (4097, 4096), (129600, 8192), (129600, 200000)])
def test_size_is_what_carve_render_carves(R, k3):
    from nerfart_amd import hip
    for max_iter in (0, 5):
        assert hip.lib.nerfart_volsdf_render_workspace_bytes(R, 128, 64, max_iter, k3) == _render(R, 128, 64, max_iter, k3)


def test_size_is_monotone_in_the_ray_count():
    from nerfart_amd import hip
    for k3 in (1, 64, 8192):
        sizes = [hip.lib.nerfart_volsdf_render_workspace_bytes(R, 128, 64, 5, k3) for R in (1, 2, 63, 64, 65, 1000, 8191, 8192, 8193, 50000, 129600, 131072)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (k3, sizes)
    print(f"  R = 129,600, 5 rounds, k3_rays_chunk = 8,192: {hip.lib.nerfart_volsdf_render_workspace_bytes(129600, 128, 64, 5, 8192) / 2 ** 30:.3f} GiB")
