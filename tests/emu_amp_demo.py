"""CPU stand-in of ``HipBackend.amp_demo_fetch``: the numpy draw table of tests/ref_amp_demo.py, the existing
emulator's ``motion_state`` / ``build_amp_obs`` on the slot times ``build_amp_obs_demo`` computes, and the ring placement.  TEST
INFRASTRUCTURE ONLY - it lets ``AmpObsDemoSource.fetch_into``, ``ReplayBuffer.store_with`` and the agents' ``device_demo_fetch``
run without a GPU."""
import torch

from tests import ref_amp_demo as RD
from tests.emu_backend import EmuBackend


class EmuAmpDemo(EmuBackend):
    name = "emu-amp-demo"

    def amp_demo_fetch(self, clips, out, ring_rows, head, n, num_steps, truncate_time, dt, local_root_obs, root_height_obs,
                       motion_ids=None, motion_times0=None, rng_state=None, clip_cdf=None, advance=True, draws_out=None,
                       head_dev=None):
        n, S = int(n), int(num_steps)
        J, K = len(clips['dof_offsets']) - 1, len(clips['key_body_ids'])
        F = 13 + 6 * J + int(clips['dof_offsets'][-1]) + 3 * K
        n_clips = clips['lengths'].numel()
        given, drawn = motion_ids is not None and motion_times0 is not None, rng_state is not None and clip_cdf is not None
        assert given != drawn and 1 <= n <= ring_rows and 0 <= head < ring_rows
        assert out.shape[0] >= ring_rows and out.shape[1] >= S * F
        if drawn:
            m, t0 = RD.ref_draws(int(rng_state[0]), int(rng_state[1]), n, clip_cdf.numpy(), clips['lengths'].numpy(),
                                 RD.np.float32(truncate_time))
            ids, t0 = torch.from_numpy(m), torch.from_numpy(t0)
            if advance:
                rng_state[1] += 1
        else:
            ids, t0 = motion_ids, motion_times0
        if draws_out is not None:
            draws_out[0].copy_(ids)
            draws_out[1].copy_(t0)
        if head_dev is not None:
            if not 0 <= int(head_dev) < ring_rows:
                return
            head = head + int(head_dev)
        ok = (ids >= 0) & (ids < n_clips)
        # AmpObsDemoSource.build_amp_obs_demo's times and chain; a skipped sample's clip is replaced, its row dropped below
        times = (t0.unsqueeze(-1) + (-float(dt) * torch.arange(0, S))).reshape(-1)
        idx = torch.where(ok, ids, torch.zeros_like(ids)).view(-1, 1).expand(n, S).reshape(-1)
        pose = self.motion_state(clips, idx.to(torch.int32), times)
        root_pos, root_rot, dof_pos, root_vel, root_ang_vel, dof_vel, key_pos = pose
        frames = torch.zeros(n * S, 1, F)
        self.build_amp_obs(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos, clips['dof_offsets'],
                           local_root_obs, root_height_obs, frames, shift=False)
        rows = (head + torch.arange(n)) % ring_rows
        out[rows[ok], :S * F] = frames.view(n, S * F)[ok]
