"""GpuWaypointEnv -- the torch-native batched environment over libamenv.so.

N independent copies of the reference's `WaypointQuadEnv` (v2/rl_env_scaledObs.py:9-231)
live in the HBM of one MI355X; `step()` is ONE HIP kernel launch on torch's current stream.
PyTorch is only the device container here (buffers, streams): all arithmetic is in the HIP
kernels behind the C ABI (include/amenv.h).  There is no CPU path.
"""
import ctypes as C

import torch

from . import _lib as L
from .action_delay import ActionDelay
from .action_history import ActionHistory
from .randomization import DynamicsRandomization
from .rate_control import RateControl
from .rotor_failure import RotorFailure
from .rotor_lag import RotorLag
from .sensor_noise import SensorNoise

# The opt-in switches, in the order the constructor applies them: keyword = attribute = the <name> of set_<name> and amenv_set_<name> ->
# (class, the method that gives its C struct; the history's argument is its row count)
_SWITCHES = {"randomization": (DynamicsRandomization, "to_c"), "rotor_lag": (RotorLag, "to_c"), "sensor_noise": (SensorNoise, "to_c"),
             "action_delay": (ActionDelay, "_as_c"), "action_history": (ActionHistory, None), "rate_control": (RateControl, "to_c"),
             "rotor_failure": (RotorFailure, "to_c")}


def _typed(who, x, cls):
    if x is not None and not isinstance(x, cls):
        raise L.AmenvError(f"{who}: expected {'an' if cls.__name__[0] in 'AEIOU' else 'a'} {cls.__name__} or None, got {type(x).__name__}")


def _dev_index(device):
    if isinstance(device, int):
        return device
    d = torch.device(device)
    if d.type != "cuda":
        raise L.AmenvError(f"GpuWaypointEnv needs a GPU device (got {d}); there is no CPU fallback")
    return d.index if d.index is not None else torch.cuda.current_device()


class GpuWaypointEnv:
    """Batched waypoint environment resident on one GPU.

    step(actions[N,4] f32 cuda) -> (obs[N,20] f32, reward[N], done[N] u8, info_bits[N] i32)
    Returned tensors are persistent output buffers, overwritten by the next call (zero-copy).
    After a step, for envs with done != 0: `terminal_obs[i]`, `ep_return[i]`, `ep_len[i]` hold
    the SB3 `terminal_observation` and Monitor `episode` r / l values.
    """

    def __init__(self, num_envs, device=0, vehicle="quad", seed=0, dtype="f32", auto_reset=True, nan_guard=False,
                 num_waypoints=1, env_id_offset=0, block_size=0, max_episode_steps=None, counter_limit=None,
                 rk4_substeps=1, task="v2", config=None, kernel="auto", ee_task=None, n_joints=None, randomization=None, rotor_lag=None,
                 sensor_noise=None, action_delay=None, action_history=None, rate_control=None, rotor_failure=None):
        switches = {"randomization": randomization, "rotor_lag": rotor_lag, "sensor_noise": sensor_noise, "action_delay": action_delay,
                    "action_history": action_history, "rate_control": rate_control, "rotor_failure": rotor_failure}
        for name, x in switches.items():   # before any device is touched
            _typed(name, x, _SWITCHES[name][0])
        self.lib = L.load()
        self.device_index = _dev_index(device)
        self.device = torch.device("cuda", self.device_index)
        if config is None:
            # task: "v2" | "v1_scaled" | "v1_raw" (which reference env file); n_joints (hexa_arm): 1..3 links of the default arm
            cfg = L.default_config(vehicle, num_envs, task, n_joints=n_joints)
            cfg.seed = seed
            cfg.dtype = L.F64 if dtype in ("f64", torch.float64) else L.F32
            cfg.flags = (L.FLAG_AUTO_RESET if auto_reset else 0) | (L.FLAG_NAN_GUARD if nan_guard else 0)
            cfg.env_id_offset = env_id_offset
            cfg.block_size = block_size
            cfg.step_kernel = L.KERNELS[kernel]   # "auto" | "lane" | "helper" | "team": which implementation of the same step runs
            if ee_task is not None:               # arm vehicles: "tool" (default) | "base" -- the point the waypoint task measures from
                cfg.task.ee_task = {"base": L.EE_TASK_BASE, "tool": L.EE_TASK_TOOL}[ee_task]
            cfg.task.rk4_substeps = rk4_substeps
            if max_episode_steps is not None:
                cfg.task.max_episode_steps = max_episode_steps
            if counter_limit is not None:
                cfg.task.counter_limit = counter_limit
            if num_waypoints != 1 and task == "v2":
                import math
                cfg.task.num_waypoints = num_waypoints
                for k in range(1, num_waypoints + 1):
                    t = k / num_waypoints
                    cfg.task.traj_sin[k - 1] = math.sin(2.0 * t * math.pi)
                    cfg.task.traj_cos[k - 1] = math.cos(t * 2.0 * math.pi)
        else:
            cfg = config
        self.cfg = cfg
        self.num_envs = cfg.num_envs
        od, ad, nf, ni = (C.c_int32() for _ in range(4))
        self.lib.amenv_dims(C.byref(cfg), C.byref(od), C.byref(ad), C.byref(nf), C.byref(ni))
        self.obs_dim, self.act_dim, self.n_float_fields, self.n_int_fields = od.value, ad.value, nf.value, ni.value
        self.state_dtype = torch.float64 if cfg.dtype == L.F64 else torch.float32
        self.bytes_per_env_step = int(self.lib.amenv_bytes_per_env_step(C.byref(cfg)))
        h = C.c_void_p()
        rc = self.lib.amenv_create(C.byref(cfg), self.device_index, C.byref(h))
        if rc != 0:
            raise L.AmenvError(f"amenv_create failed ({rc}): {self.lib.amenv_last_error(None).decode()}")
        self._h = h
        n, dev = self.num_envs, self.device
        self.obs = torch.zeros(n, self.obs_dim, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(n, dtype=self.state_dtype, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.info_bits = torch.zeros(n, dtype=torch.int32, device=dev)
        self.terminal_obs = torch.zeros(n, self.obs_dim, dtype=torch.float32, device=dev)
        self.ep_return = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self.kernel_name = self.lib.amenv_kernel_name(self._h).decode()
        self.n_rotors = int(cfg.vehicle.n_rotors)
        for name, x in switches.items():
            setattr(self, name, None)
            if x is not None:
                getattr(self, "set_" + name)(x)

    # ------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        if rc != 0:
            raise L.AmenvError(f"{what} failed ({rc}): {self.lib.amenv_last_error(self._h).decode()}")

    def _set_switch(self, name, x):
        """set_<name>(x) of a struct-valued switch: the type check, amenv_set_<name> with x's C struct (NULL for None), the attribute, the
        kernel's name."""
        cls, to_c = _SWITCHES[name]
        _typed("set_" + name, x, cls)
        c = None if x is None else getattr(x, to_c)()
        self._check(getattr(self.lib, "amenv_set_" + name)(self._h, None if c is None else C.byref(c)), "amenv_set_" + name)
        setattr(self, name, x)
        self.kernel_name = self.lib.amenv_kernel_name(self._h).decode()

    def _actions(self, actions, lead=()):
        want = tuple(lead) + (self.num_envs, self.act_dim)
        if actions.device != self.device or actions.dtype != torch.float32 or tuple(actions.shape) != want or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.float32).reshape(want).contiguous()
        if actions.data_ptr() % 16:    # e.g. a row of a [T, N, A] tensor with odd N*A: the kernels want 16-byte aligned buffers
            actions = actions.clone()
        return actions

    def reseed(self, seed):
        """Re-key the reset RNG for episodes started from now on."""
        self._check(self.lib.amenv_set_seed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF), "amenv_set_seed")
        self.cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def set_randomization(self, r):
        """Per-episode dynamics randomisation (a `DynamicsRandomization`, or None = the nominal vehicle; rigid vehicles with 4 or 6 rotors,
        not with kernel="team").  The factors are a pure function of (seed, env id, episode, ranges): new ranges apply from the next
        launch on, to the episodes already running too."""
        self._set_switch("randomization", r)

    def dynamics_factors(self):
        """[N, 2 + n_rotors] f32 on this env's device: km, kI, s_0.. of every env's current episode (all 1 without randomisation)."""
        out = torch.empty(self.num_envs, 2 + self.n_rotors, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_dynamics_factors(self._h, C.c_void_p(out.data_ptr()), self._stream()), "amenv_dynamics_factors")
        return out

    def set_rotor_lag(self, lag):
        """First-order rotor lag (a `RotorLag`, or None = rotors deliver their command at once; rigid vehicles with 4 or 6 rotors, not
        with kernel="team").  Turning it on sets every env's rotor state to the nominal hover command; new time constants on an env where
        it is on keep the states and apply from the next launch.  A configuration call: it may allocate and synchronise."""
        self._set_switch("rotor_lag", lag)

    def rotor_state(self):
        """[N, n_rotors] of the state dtype: every rotor's state w = sqrt(delivered thrust).  Needs the rotor lag on."""
        out = torch.empty(self.num_envs, self.n_rotors, dtype=self.state_dtype, device=self.device)
        self._check(self.lib.amenv_get_rotor_state(self._h, C.c_void_p(out.data_ptr()), self._stream()), "amenv_get_rotor_state")
        return out

    def set_rotor_state(self, w):
        """The inverse of rotor_state(): parity injection, checkpoint / restore."""
        t = torch.as_tensor(w).to(device=self.device, dtype=self.state_dtype).contiguous()
        if tuple(t.shape) != (self.num_envs, self.n_rotors):
            raise L.AmenvError(f"set_rotor_state: expected shape {(self.num_envs, self.n_rotors)}, got {tuple(t.shape)}")
        self._check(self.lib.amenv_set_rotor_state(self._h, C.c_void_p(t.data_ptr()), self._stream()), "amenv_set_rotor_state")
        torch.cuda.current_stream(self.device).synchronize()   # the staging tensor stays alive until the copy has run

    def set_sensor_noise(self, noise):
        """Sensor noise on every observation row (a `SensorNoise`, or None = exact observations; fp32 rigid vehicles with 4 or 6 rotors,
        not with kernel="team").  A pure function of (seed, env id, episode, step): nothing is stored, it applies from the next launch,
        and observe() repeats the row the last step returned.  Reward, termination, get_state() and stats() stay exact."""
        self._set_switch("sensor_noise", noise)

    def sensor_noise_samples(self):
        """[N, 12] f32 on this env's device: the unit samples of every env's current (episode, step) -- position 0..2, velocity 3..5,
        body rate 6..8, attitude 9..11 -- drawn by the kernels' own device function."""
        out = torch.empty(self.num_envs, 12, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_sensor_noise_samples(self._h, C.c_void_p(out.data_ptr()), self._stream()), "amenv_sensor_noise_samples")
        return out

    def set_action_delay(self, delay):
        """Per-episode actuation latency (an `ActionDelay`, or None = every action is applied in the step that receives it; fp32 rigid
        vehicles with 4 or 6 rotors, not with kernel="team").  Turning it on draws every env's delay for its current episode and fills its
        history with hover rows; a new range on an env where it is on keeps both and applies to the episodes that start afterwards.  A
        configuration call: it may allocate and synchronise."""
        self._set_switch("action_delay", delay)

    def set_action_history(self, history):
        """Action history in the observation rows (an `ActionHistory`, or None = the task's rows; fp32 rigid vehicles with 4 or 6 rotors, not
        with kernel="team").  While it is on every row this env publishes is the task's row followed by the last `rows` action rows the env
        was given, most recent first (hover rows where the episode is younger): `obs_dim` = 20 (17 on the v1 tasks) + 4 rows.  `obs` and
        `terminal_obs` are re-allocated at the new width (zeros: `observe()` returns the current rows).  A configuration call: it may
        allocate and synchronise."""
        _typed("set_action_history", history, ActionHistory)
        self._check(self.lib.amenv_set_action_history(self._h, 0 if history is None else history.rows), "amenv_set_action_history")
        self.action_history = history
        self.obs_dim = int(self.lib.amenv_obs_dim(self._h))
        self.obs = torch.zeros(self.num_envs, self.obs_dim, dtype=torch.float32, device=self.device)
        self.terminal_obs = torch.zeros(self.num_envs, self.obs_dim, dtype=torch.float32, device=self.device)
        self.kernel_name = self.lib.amenv_kernel_name(self._h).decode()

    def set_rate_control(self, rate):
        """Body-rate actions (a `RateControl`, or None = entries 1..3 of an action row are moments; fp32 rigid vehicles with 4 or 6 rotors,
        not with kernel="team").  While it is on, entries 1..3 are rate commands in units of `max_rate` and a proportional rate loop on the
        nominal inertia, inside the step and behind the latency, forms the moments.  The rows of the action history and of PPO's buffers stay
        the commands as given.  No state, no allocation: it applies from the next launch."""
        _typed("set_rate_control", rate, RateControl)
        if rate is not None:
            rate.validate(self.cfg.task.dt)
        self._set_switch("rate_control", rate)

    def moment_actions(self, actions):
        """[N, 4] f32: the rows [a_0, a'_x, a'_y, a'_z] the rate loop forms from the command rows `actions` and every env's CURRENT body
        rates, by the kernels' own device function (the latency is ignored: it converts the rows it is given).  Stepping a twin env without
        rate control with them reproduces this env's next step.  Needs rate control on."""
        a = self._actions(actions)
        out = torch.empty(self.num_envs, 4, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_rate_moment_actions(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()), self._stream()),
                    "amenv_rate_moment_actions")
        return out

    def set_rotor_failure(self, failure):
        """Per-episode rotor failure (a `RotorFailure`, or None = every rotor delivers its factor for the whole episode; rigid vehicles with
        4 or 6 rotors, not with kernel="team").  With its probability an episode has one failure: from the drawn onset step on, the drawn
        rotor delivers only the drawn fraction of its thrust.  A pure function of (seed, env id, episode, parameters): nothing is stored,
        new parameters apply from the next launch, to the episodes already running too.  The failure is not observed."""
        _typed("set_rotor_failure", failure, RotorFailure)
        if failure is not None:
            failure.validate(self.n_rotors)
        self._set_switch("rotor_failure", failure)

    def rotor_failure_state(self):
        """(plan [N, 2] int32, factors [N, n_rotors] f32): every env's failed rotor (-1: its current episode has none) and onset step, and
        the multiplier on each rotor's thrust factor in effect for the NEXT step (the remaining fraction on the failed rotor once the env's
        step has reached the onset, else 1), by the kernels' own device functions.  Needs the rotor failure on."""
        plan = torch.empty(self.num_envs, 2, dtype=torch.int32, device=self.device)
        factors = torch.empty(self.num_envs, self.n_rotors, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_rotor_failure_state(self._h, C.c_void_p(plan.data_ptr()), C.c_void_p(factors.data_ptr()), self._stream()),
                    "amenv_rotor_failure_state")
        return plan, factors

    def action_delay_state(self):
        """(d [N] int32, recent [N, 8, 4] f32): every env's delay and the last 8 action rows it was given, in age order (recent[:, k] was
        given k + 1 steps ago; the hover row where the episode is younger).  Needs the action delay or the action history on."""
        d = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        recent = torch.empty(self.num_envs, L.MAX_ACTION_DELAY, 4, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_get_action_delay_state(self._h, C.c_void_p(d.data_ptr()), C.c_void_p(recent.data_ptr()), self._stream()),
                    "amenv_get_action_delay_state")
        return d, recent

    def set_action_delay_state(self, d, recent):
        """The inverse of action_delay_state(): checkpoint / restore, parity injection.  d outside 0..8 is clamped."""
        n = self.num_envs
        dt = torch.as_tensor(d).to(device=self.device, dtype=torch.int32).contiguous()
        rt = torch.as_tensor(recent).to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(dt.shape) != (n,) or tuple(rt.shape) != (n, L.MAX_ACTION_DELAY, 4):
            raise L.AmenvError(f"set_action_delay_state: expected shapes {(n,)} and {(n, L.MAX_ACTION_DELAY, 4)}, got {tuple(dt.shape)} and {tuple(rt.shape)}")
        if rt.data_ptr() % 16:
            rt = rt.clone()
        self._check(self.lib.amenv_set_action_delay_state(self._h, C.c_void_p(dt.data_ptr()), C.c_void_p(rt.data_ptr()), self._stream()),
                    "amenv_set_action_delay_state")
        torch.cuda.current_stream(self.device).synchronize()   # the staging tensors stay alive until the copy has run

    def reset(self, mask=None):
        """WaypointQuadEnv.reset (v2/rl_env_scaledObs.py:40-79) for all envs, or those with mask != 0."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._check(self.lib.amenv_reset(self._h, None if m is None else C.c_void_p(m.data_ptr()), C.c_void_p(self.obs.data_ptr()),
                                         self._stream()), "amenv_reset")
        return self.obs

    def step(self, actions):
        """WaypointQuadEnv.step (v2/rl_env_scaledObs.py:123-196) for all N envs: one kernel launch."""
        a = self._actions(actions)
        self._check(self.lib.amenv_step(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(self.obs.data_ptr()),
                                        C.c_void_p(self.reward.data_ptr()), C.c_void_p(self.done.data_ptr()),
                                        C.c_void_p(self.info_bits.data_ptr()), C.c_void_p(self.terminal_obs.data_ptr()),
                                        C.c_void_p(self.ep_return.data_ptr()), C.c_void_p(self.ep_len.data_ptr()), self._stream()),
                    "amenv_step")
        return self.obs, self.reward, self.done, self.info_bits

    def step_into(self, actions, obs, reward, done):
        """step() writing obs [N,obs_dim] f32, reward [N], done [N] u8 straight into caller tensors (e.g. rows of a rollout
        buffer) instead of the persistent output buffers; info_bits / terminal_obs / ep_return / ep_len as in step()."""
        a = self._actions(actions)
        n = self.num_envs
        ok = (obs.device == self.device and obs.dtype == torch.float32 and obs.is_contiguous() and tuple(obs.shape) == (n, self.obs_dim)
              and reward.device == self.device and reward.dtype == self.state_dtype and reward.is_contiguous() and reward.numel() == n
              and done.device == self.device and done.dtype == torch.uint8 and done.is_contiguous() and done.numel() == n)
        if not ok:
            raise L.AmenvError("step_into: obs/reward/done must be contiguous tensors of this env's device, dtype and shape")
        self._check(self.lib.amenv_step(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(obs.data_ptr()),
                                        C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()),
                                        C.c_void_p(self.info_bits.data_ptr()), C.c_void_p(self.terminal_obs.data_ptr()),
                                        C.c_void_p(self.ep_return.data_ptr()), C.c_void_p(self.ep_len.data_ptr()), self._stream()),
                    "amenv_step")
        return obs, reward, done, self.info_bits

    def step_timed(self, actions):
        """step() that also returns the device-side duration (us) of that one kernel launch (synchronises)."""
        a = self._actions(actions)
        us = C.c_float()
        self._check(self.lib.amenv_step_timed(self._h, C.c_void_p(a.data_ptr()), C.c_void_p(self.obs.data_ptr()),
                                              C.c_void_p(self.reward.data_ptr()), C.c_void_p(self.done.data_ptr()),
                                              C.c_void_p(self.info_bits.data_ptr()), C.c_void_p(self.terminal_obs.data_ptr()),
                                              C.c_void_p(self.ep_return.data_ptr()), C.c_void_p(self.ep_len.data_ptr()), self._stream(),
                                              C.byref(us)), "amenv_step_timed")
        return us.value

    def rollout(self, actions, want_obs=True, want_flags=True):
        """T open-loop steps in one launch; actions [T,N,4].  Returns dict of [T,N,...] tensors."""
        T = int(actions.shape[0])
        a = self._actions(actions, lead=(T,))
        n, dev = self.num_envs, self.device
        out = dict(reward=torch.empty(T, n, dtype=self.state_dtype, device=dev))
        if want_obs:
            out["obs"] = torch.empty(T, n, self.obs_dim, dtype=torch.float32, device=dev)
        if want_flags:
            out["done"] = torch.empty(T, n, dtype=torch.uint8, device=dev)
            out["info_bits"] = torch.empty(T, n, dtype=torch.int32, device=dev)
        p = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None
        self._check(self.lib.amenv_rollout(self._h, T, C.c_void_p(a.data_ptr()), p("obs"), p("reward"), p("done"), p("info_bits"),
                                           self._stream()), "amenv_rollout")
        return out

    def rollout_policy(self, flat_params, n_steps, seed, draw0, obs, actions, logp, values, rewards, dones, info_bits=None, terminal_obs=None,
                       obs_normalizer=None, update_normalizer=True):
        """T closed-loop steps in ONE launch: obs -> actor / critic MLPs (bf16 matrix cores) -> Gaussian sample -> clip -> env step,
        writing SB3's rollout-buffer rows: obs [T+1,N,OD] (row 0 = observation at entry), actions [T,N,A] raw samples, logp / values /
        rewards [T,N] f32, dones [T,N] u8, optionally info_bits [T,N] i32 and terminal_obs [T,N,OD].  Caller-owned contiguous tensors on
        this env's device.  Built for fp32 envs: the rigid vehicles with 4 or 6 rotors on every task, and the hexacopter with a 1-, 2- or
        3-link arm (any joint axes) on the v2 task with 1..4 waypoints (include/amenv.h amenv_rollout_policy).  OD and A are this env's
        obs_dim / act_dim: a shorter arm's rows are as amenv_step publishes them (23 + 2 n / 4 + n wide).

        obs_normalizer (an `ObsNormalizer` of dim obs_dim on this device; rigid vehicles only): the normaliser runs INSIDE the launch
        (amenv_rollout_policy_norm) with its clip_obs / epsilon.  Its statistics are FROZEN for the launch: every row written (obs,
        terminal_obs) and the policy's input are normalised with the statistics at entry, bit-identical to `obs_normalizer.normalize(raw)`.
        update_normalizer: afterwards the statistics have merged the raw rows 1..T (not row 0, not the terminal rows), as T per-step
        VecNormalize updates would to fp64 rounding; False (evaluation) leaves them untouched."""
        T, n = int(n_steps), self.num_envs
        want = {"obs": ((T + 1, n, self.obs_dim), torch.float32), "actions": ((T, n, self.act_dim), torch.float32), "logp": ((T, n), torch.float32),
                "values": ((T, n), torch.float32), "rewards": ((T, n), torch.float32), "dones": ((T, n), torch.uint8)}
        got = {"obs": obs, "actions": actions, "logp": logp, "values": values, "rewards": rewards, "dones": dones}
        if info_bits is not None:      # optional outputs are written [T,N] / [T,N,OD] by the kernel all the same: check them like the rest
            want["info_bits"] = ((T, n), torch.int32); got["info_bits"] = info_bits
        if terminal_obs is not None:
            want["terminal_obs"] = ((T, n, self.obs_dim), torch.float32); got["terminal_obs"] = terminal_obs
        for k, (shape, dt) in want.items():
            t = got[k]
            if t.device != self.device or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise L.AmenvError(f"rollout_policy: {k} must be a contiguous {dt} tensor of shape {shape} on {self.device}")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        fp = flat_params.detach()
        if fp.device != self.device or fp.dtype != torch.float32 or not fp.is_contiguous():
            raise L.AmenvError("rollout_policy: flat_params must be a contiguous fp32 tensor on this env's device")
        tail = (T, p(fp), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw0) & 0xFFFFFFFF, p(obs), p(actions), p(logp), p(values), p(rewards), p(dones),
                p(info_bits), p(terminal_obs), self._stream())
        if obs_normalizer is None:
            self._check(self.lib.amenv_rollout_policy(self._h, *tail), "amenv_rollout_policy")
        else:
            self._check(self.lib.amenv_rollout_policy_norm(self._h, obs_normalizer._h, 1 if update_normalizer else 0, float(obs_normalizer.clip_obs),
                                                           float(obs_normalizer.epsilon), *tail), "amenv_rollout_policy_norm")

    def evaluate_policy(self, flat_params, episodes_per_env, max_steps=None, deterministic=True, seed=0, draw0=0, obs_normalizer=None, reset=True):
        """Closed-loop EVALUATION in ONE launch (amenv_evaluate_policy, include/amenv.h): the loop of rollout_policy() with the episode
        accounting on the device and no per-step output.  Every env counts the first `episodes_per_env` episodes that end in it; the launch
        ends when all have, or after `max_steps` steps (default: episodes_per_env * (max_episode_steps + 2)).  deterministic: the applied
        action is clip(mean); otherwise rollout_policy()'s sample under (seed, draw0).  obs_normalizer: used FROZEN, never updated.
        reset=True calls reset() first; with reset=False the episodes already running count when they end.

        Returns device tensors, without a sync: {"returns": [N, 2] f64 (sum, sum of squares of the counted episodes' returns), "counts":
        [N, 6] i32 (EVAL_COUNT_COLS: episodes, length_sum, success, crashed, out_of_bounds, truncated), "steps_run": 0-dim i32}.
        Afterwards the env is wherever its lanes stopped (reset() before anything that needs a defined start); stats() is untouched."""
        if max_steps is None:
            max_steps = int(episodes_per_env) * (int(self.cfg.task.max_episode_steps) + 2)
        fp = flat_params.detach()
        if fp.device != self.device or fp.dtype != torch.float32 or not fp.is_contiguous():
            raise L.AmenvError("evaluate_policy: flat_params must be a contiguous fp32 tensor on this env's device")
        if reset:
            self.reset()
        n, dev = self.num_envs, self.device
        out = {"returns": torch.empty(n, 2, dtype=torch.float64, device=dev), "counts": torch.empty(n, L.EVAL_COUNT_COLS, dtype=torch.int32, device=dev),
               "steps_run": torch.empty((), dtype=torch.int32, device=dev)}
        nz = obs_normalizer
        self._check(self.lib.amenv_evaluate_policy(self._h, None if nz is None else nz._h, 0.0 if nz is None else float(nz.clip_obs),
                                                   0.0 if nz is None else float(nz.epsilon), C.c_void_p(fp.data_ptr()), 1 if deterministic else 0,
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw0) & 0xFFFFFFFF, int(episodes_per_env), int(max_steps),
                                                   C.c_void_p(out["returns"].data_ptr()), C.c_void_p(out["counts"].data_ptr()),
                                                   C.c_void_p(out["steps_run"].data_ptr()), self._stream()), "amenv_evaluate_policy")
        return out

    def observe(self):
        o = torch.empty(self.num_envs, self.obs_dim, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_observe(self._h, C.c_void_p(o.data_ptr()), self._stream()), "amenv_observe")
        return o

    def ee_position(self):
        """World position [N,3] f32 of the arm's tool point (forward kinematics of the current state; the body origin without an arm)."""
        o = torch.empty(self.num_envs, 3, dtype=torch.float32, device=self.device)
        self._check(self.lib.amenv_ee_position(self._h, C.c_void_p(o.data_ptr()), self._stream()), "amenv_ee_position")
        return o

    def get_state(self):
        """(fstate [n_float_fields,N] of the state dtype, istate [4,N] int32): the SoA episode state."""
        f = torch.empty(self.n_float_fields, self.num_envs, dtype=self.state_dtype, device=self.device)
        i = torch.empty(self.n_int_fields, self.num_envs, dtype=torch.int32, device=self.device)
        self._check(self.lib.amenv_get_state(self._h, C.c_void_p(f.data_ptr()), C.c_void_p(i.data_ptr()), self._stream()), "amenv_get_state")
        return f, i

    def set_state(self, fstate=None, istate=None):
        f = i = None
        if fstate is not None:
            f = torch.as_tensor(fstate).to(device=self.device, dtype=self.state_dtype).contiguous()
            assert tuple(f.shape) == (self.n_float_fields, self.num_envs), f.shape
        if istate is not None:
            i = torch.as_tensor(istate).to(device=self.device, dtype=torch.int32).contiguous()
            assert tuple(i.shape) == (self.n_int_fields, self.num_envs), i.shape
        self._check(self.lib.amenv_set_state(self._h, None if f is None else C.c_void_p(f.data_ptr()),
                                             None if i is None else C.c_void_p(i.data_ptr()), self._stream()), "amenv_set_state")
        # keep the staging tensors alive until the copy has been enqueued AND executed
        torch.cuda.current_stream(self.device).synchronize()

    def stats(self, reset=False):
        s = L.Stats()
        self._check(self.lib.amenv_stats_read(self._h, C.byref(s), 1 if reset else 0, self._stream()), "amenv_stats_read")
        d = {k: int(getattr(s, k)) for k, _ in L.Stats._fields_}
        d["return_sum"] = d.pop("return_sum_q10") / 1024.0
        return d

    def close(self):
        if getattr(self, "_h", None):
            self.lib.amenv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
