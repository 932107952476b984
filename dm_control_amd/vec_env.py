"""Gym-style vector environment over the batched suite environments.

Calling convention of the reference's only data-parallel mechanism,
`SubprocVecEnv` (/root/reference/dm_control/scripts/vec_env.py:127-135,
346-352, 447-472): `reset() -> obs[B, D]`; `step(actions[B, nu]) ->
(obs[B, D], rewards[B], dones[B], infos)`; an env that finishes is reset
inside `step` and its last observation is reported as
`info['terminal_observation']`.  Here the B "workers" are lanes of one kernel
launch instead of OS processes, so stepping needs no pipes or pickling.

Two I/O modes:
  * numpy (default): actions are host arrays, results are host arrays; every
    step costs one H2D and a few D2H copies (PCIe-inclusive path).
  * torch (`torch_io=True`): actions are CUDA tensors read in place, results
    are CUDA tensors aliasing the kernel's output buffers, everything runs on
    torch's current stream -- no host round trip in the loop.

By default the B envs share one episode (they start and end together).  With
`per_env_episodes=True` every env has its own, like the workers of
`SubprocVecEnv`: the step kernel counts each env's steps and raises its done
bits on the device, `dones` is per env, an env that is done -- at the time limit
or because its state went bad -- is re-initialised alone (`Task.reset_done`) and
reports the first observation of its new episode, and `episode_offsets`
staggers the first episodes.  A bad state never raises in this mode.
"""

import math

import numpy as np

from dm_control_amd import suite
from dm_control_amd import wrapper
from dm_control_amd.rl import control


class VecEnv:
  """B synchronous suite environments with auto-reset."""

  def __init__(self, domain_name, task_name, num_envs, seed=None,
               device=0, precision='f32', torch_io=False, task_kwargs=None,
               environment_kwargs=None, per_env=(), per_env_episodes=False,
               episode_offsets=None, rollout=False, population=False):
    """rollout: build the rollout variant of the step kernel, for `rollout()`
    (torch mode, lock-step episodes, one-env-per-lane domains).
    population: with rollout=True, the rollout build that takes an
    `rl.policy.MLPPopulation`: one policy per group of consecutive envs.
    per_env_episodes: every env ends and restarts its episodes on its own
    (needs device_init, the default of torch mode).  episode_offsets: None,
    'staggered' (env e starts e/B of the way into its first episode) or int [B]:
    the step count every env's first episode starts with after `reset()`."""
    env_kw = dict(environment_kwargs or {})
    if per_env:        # model fields read per env (Physics.set_model_params)
      env_kw['per_env'] = tuple(per_env)
    env_kw.update(batch_size=int(num_envs), device=device,
                  precision=precision, flat_observation=True)
    self._rollout = bool(rollout or env_kw.get('rollout'))
    if self._rollout:
      if not torch_io:
        raise ValueError('rollout=True needs torch_io=True: a rollout records into '
                         'CUDA tensors')
      if per_env_episodes:
        raise ValueError('rollout=True is lock-step: not with per_env_episodes=True')
      env_kw['rollout'] = True
      self._policy_cache = {}
    self._population = bool(population or env_kw.get('population'))
    if self._population:
      if not self._rollout:
        raise ValueError('population=True is a variant of the rollout build: it needs '
                         'rollout=True')
      env_kw['population'] = True
    self._member_of_env, self._members = None, 0
    env_kw.setdefault('device_init', bool(torch_io))
    task_kw = dict(task_kwargs or {})
    task_kw.setdefault('random', seed)
    self._env = suite.load(domain_name, task_name, task_kwargs=task_kw,
                           environment_kwargs=env_kw)
    self.num_envs = int(num_envs)
    self._physics = self._env.physics
    self._batch = self._physics.batch
    self._torch = bool(torch_io)
    self._nsub = self._env._n_sub_steps          # pylint: disable=protected-access
    self._step_limit = self._env._step_limit     # pylint: disable=protected-access
    self._count = 0
    self._per_env = bool(per_env_episodes)
    if self._per_env:
      if not env_kw['device_init']:
        raise ValueError('per_env_episodes=True needs device_init=True: the host-RNG '
                         'recipes redraw the whole batch')
      limit = 0 if math.isinf(self._step_limit) else max(1, int(math.ceil(self._step_limit)))
      if episode_offsets is None:
        offsets = np.zeros(self.num_envs, np.int32)
      elif isinstance(episode_offsets, str):
        if episode_offsets != 'staggered' or not limit:
          raise ValueError("episode_offsets: None, 'staggered' (with a time limit) or int [B]")
        offsets = (np.arange(self.num_envs, dtype=np.int64)*limit//self.num_envs).astype(np.int32)
      else:
        offsets = np.asarray(episode_offsets, np.int32)
        if offsets.shape != (self.num_envs,):
          raise ValueError('episode_offsets must have shape (%d,)' % self.num_envs)
      self._offsets = offsets
      self._physics.enable_episodes(limit)
      # the humanoid's rejection loop depends on the data: it runs only when needed
      self._pass_needs_done = domain_name == 'humanoid'
    elif episode_offsets is not None:
      raise ValueError('episode_offsets needs per_env_episodes=True')
    spec = self._env.action_spec()
    self.action_low, self.action_high = spec.minimum, spec.maximum
    self.action_dim = int(spec.shape[0])
    self.observation_dim = int(self._batch.model.info.nobs)
    if self._torch:
      from dm_control_amd import torch_io as tio
      tio.use_current_stream(self._batch)
      self._obs_t = tio.field_tensor(self._batch, wrapper.FIELD_OBS)
      self._rew_t = tio.field_tensor(self._batch, wrapper.FIELD_REWARD)
      if self._per_env:
        self._done_t = tio.episode_tensor(self._batch, wrapper.EPISODE_DONE)

  @property
  def environment(self):
    return self._env

  # -- numpy mode -------------------------------------------------------------
  def _obs(self, timestep):
    return timestep.observation[control.FLAT_OBSERVATION_KEY]

  def reset(self):
    """Starts new episodes everywhere; returns obs [B, D]."""
    if self._per_env:
      with self._physics.reset_context():
        self._env.task.initialize_episode(self._physics)
      self._batch.episode_write(wrapper.EPISODE_STEP, self._offsets)
      return self._obs_t.clone() if self._torch else self._physics.fused_observation()
    if self._torch:
      return self._reset_torch()
    self._count = 0
    return self._obs(self._env.reset())

  def step(self, actions):
    """-> (obs [B, D], rewards [B], dones [B], infos list of dicts)."""
    if self._per_env:
      return self._step_per_env_torch(actions) if self._torch else self._step_per_env(actions)
    if self._torch:
      return self._step_torch(actions)
    ts = self._env.step(actions)
    infos = [{} for _ in range(self.num_envs)]
    dones = np.full(self.num_envs, ts.last())
    rewards = np.asarray(ts.reward, np.float64)
    obs = self._obs(ts)
    if ts.last():
      for i in range(self.num_envs):
        infos[i]['terminal_observation'] = obs[i].copy()
      obs = self._obs(self._env.reset())          # vec_env.py:346-352
    return obs, rewards, dones, infos

  # -- per-env episodes -----------------------------------------------------------
  def _step_per_env(self, actions):
    physics, task = self._physics, self._env.task
    task.before_step(actions, physics)
    physics.step(self._nsub, check=False)
    obs, rewards = physics.fused_observation(), physics.fused_reward()
    done = physics.episode_done()
    infos = [{'bad_state': bool(d & wrapper.DONE_BAD_STATE)} for d in done]
    if done.any():
      for i in np.nonzero(done)[0]:
        infos[i]['terminal_observation'] = obs[i].copy()
      task.reset_done(physics)
      obs = physics.fused_observation()
    return obs, rewards, done != 0, infos

  def _step_per_env_torch(self, actions):
    physics = self._physics
    self._launch_torch(actions)
    rewards = self._rew_t.clone()
    dones = self._done_t != 0
    infos = {'terminal_observation': self._obs_t.clone(),
             'bad_state': (self._done_t & wrapper.DONE_BAD_STATE) != 0}
    # The reset pass is issued every step without asking the device who is done:
    # its launches find an empty mask and exit.
    if not self._pass_needs_done or bool(dones.any()):
      self._env.task.reset_done(physics)
    return self._obs_t.clone(), rewards, dones, infos

  # -- torch mode ---------------------------------------------------------------
  def _launch_torch(self, actions):
    if not actions.is_cuda:
      raise ValueError('torch_io=True expects CUDA action tensors')
    a = actions.to(self._obs_t.dtype)
    if a.shape != (self.num_envs, self.action_dim):
      raise ValueError('actions must have shape (%d, %d)'
                       % (self.num_envs, self.action_dim))
    if a.stride(1) != 1:
      a = a.contiguous()
    self._keepalive = a
    self._physics.set_control_device(a.data_ptr(), a.stride(1), a.stride(0))
    self._physics.step(self._nsub, check=False)

  def _reset_torch(self):
    physics = self._physics
    with physics.reset_context():
      self._env.task.initialize_episode(physics)
    self._count = 0
    return self._obs_t.clone()

  def _step_torch(self, actions):
    import torch
    self._launch_torch(actions)
    self._count += 1
    done = self._count >= self._step_limit
    rewards = self._rew_t.clone()
    dones = torch.full((self.num_envs,), bool(done), device=rewards.device)
    infos = {}
    if done:
      infos['terminal_observation'] = self._obs_t.clone()
      obs = self._reset_torch()
    else:
      obs = self._obs_t.clone()
    return obs, rewards, dones, infos

  # -- rollouts -------------------------------------------------------------------
  @property
  def member_of_env(self):
    """int64 [B] on the device: the member env e acted with in the last rollout over
    a population (e // (B // P)); per-member fitness is then one
    `index_add_(0, member_of_env, episode_return)`, or `view(P, -1).mean(1)`."""
    if self._member_of_env is None:
      raise ValueError('member_of_env is set by a rollout over a population')
    return self._member_of_env

  def _policy_device(self, policy):
    """(device pointer, widths[, members]) of `policy`: uploaded once per policy
    object and again after its `update_`; a `from_device` population is read in place."""
    import torch
    from dm_control_amd.rl import policy as policy_lib
    members = None
    if isinstance(policy, policy_lib.MLPPopulation):
      members = policy.num_members
      if not self._population:
        raise ValueError('a population of policies needs VecEnv(..., rollout=True, '
                         'population=True)')
      if self.num_envs % members:
        raise ValueError('%d members do not divide the %d envs' % (members, self.num_envs))
      if self._members != members:
        self._members = members
        self._member_of_env = torch.arange(
            self.num_envs, device=self._obs_t.device)//(self.num_envs//members)
    if policy.obs_dim != self.observation_dim or policy.action_dim != self.action_dim:
      raise ValueError('the policy maps %d -> %d values, the env %d -> %d'
                       % (policy.obs_dim, policy.action_dim, self.observation_dim,
                          self.action_dim))
    if members is not None and policy.device_tensor is not None:
      flat = policy.device_tensor
      if flat.dtype != self._obs_t.dtype or flat.device != self._obs_t.device:
        raise ValueError('the population tensor must be %s on %s, the env\'s own'
                         % (self._obs_t.dtype, self._obs_t.device))
      return flat.data_ptr(), policy.widths, members
    held = self._policy_cache.get(id(policy))
    if held is None or held[0] is not policy or held[1] != policy.version:
      flat = torch.from_numpy(policy.packed(self._physics.dtype)).to(self._obs_t.device)
      held = (policy, policy.version, flat)
      self._policy_cache[id(policy)] = held
    if members is not None:
      return held[2].data_ptr(), policy.widths, members
    return held[2].data_ptr(), policy.widths

  def rollout(self, T, policy=None, actions=None, noise=None):
    """Up to `T` control steps in one kernel launch per 64 steps, no host round
    trip in between (`VecEnv(..., torch_io=True, rollout=True)`).

    policy: an `rl.policy.MLPPolicy`, or on a `population=True` env an
    `rl.policy.MLPPopulation` of P members (env e acts with member e // (B // P),
    `member_of_env`), evaluated by the step kernel on each env's observation:
    a_t = policy(o_t) + noise[t], `noise` an optional CUDA tensor [T, B, nu].  Without a policy, `actions` [T, B, nu] is the action sequence
    (open loop).  Runs n = min(T, steps left in the episode) steps and returns a
    dict of CUDA tensors: obs [n, B, D] (obs[t]: the observation after step t),
    actions [n, B, nu], rewards [n, B], dones [n, B] (the last row true when the
    time limit was reached), next_obs [B, D] (what to act on next: after a reset
    the new episode's first observation) and, when the episode ended,
    terminal_observation [B, D]."""
    import torch
    if not self._rollout:
      raise ValueError('rollout() needs VecEnv(..., torch_io=True, rollout=True)')
    if (policy is None) == (actions is None):
      raise ValueError('pass either a policy (closed loop) or actions (open loop)')
    if noise is not None and policy is None:
      raise ValueError('noise is added to a policy; without one pass `actions`')
    left = self._step_limit - self._count
    n = int(T) if math.isinf(left) else int(min(int(T), max(1, math.ceil(left))))
    if n < 1:
      raise ValueError('T must be at least 1')
    B, D, nu = self.num_envs, self.observation_dim, self.action_dim
    dtype, dev = self._obs_t.dtype, self._obs_t.device
    ctrl = None
    seq = actions if policy is None else noise
    if seq is not None:
      if not seq.is_cuda or seq.dim() != 3 or seq.shape[0] < n or seq.shape[1:] != (B, nu):
        raise ValueError('expected a CUDA tensor [>= %d, %d, %d]' % (n, B, nu))
      seq = seq[:n].to(dtype).contiguous()
      ctrl = (seq.data_ptr(), 1, nu, B*nu)
    out = {'obs': torch.empty(n, B, D, dtype=dtype, device=dev),
           'actions': torch.empty(n, B, nu, dtype=dtype, device=dev),
           'rewards': torch.empty(n, B, dtype=dtype, device=dev)}
    self._physics.rollout_device(
        n, self._nsub, ctrl=ctrl,
        policy=None if policy is None else self._policy_device(policy),
        obs_out=(out['obs'].data_ptr(), B*D), reward_out=(out['rewards'].data_ptr(), B),
        action_out=(out['actions'].data_ptr(), B*nu))
    self._keepalive = seq
    self._count += n
    done = self._count >= self._step_limit
    out['dones'] = torch.zeros(n, B, dtype=torch.bool, device=dev)
    if done:
      out['dones'][-1] = True
      out['terminal_observation'] = self._obs_t.clone()
      out['next_obs'] = self._reset_torch()
    else:
      out['next_obs'] = self._obs_t.clone()
    return out

  def close(self):
    self._physics.free()
