"""A small MLP policy that the step kernel of a rollout build evaluates on the
device (`VecEnv.rollout`, `Physics.rollout_device`, `dmc_batch_rollout`).

One or two tanh layers and a linear output layer over the flat observation,
weights shared by the batch.  The kernel reads them as one flat array in the code
object's `real` type: per layer W[out][in] row-major, then b[out].

`MLPPopulation` is P such policies of one shape for a population build
(`VecEnv(..., rollout=True, population=True)`, `dmc_batch_rollout_population`): env e
of B acts with member e // (B // P).  The kernel reads [nparams, P], one column per
member, rows in the packed order of a single policy.
"""

import numpy as np


class MLPPolicy:
  """`MLPPolicy(weights, biases)`: weights[l] is [out_l, in_l], biases[l] is
  [out_l]; every layer but the last is followed by tanh."""

  def __init__(self, weights, biases):
    weights = [np.array(w, np.float64) for w in weights]
    biases = [np.array(b, np.float64) for b in biases]
    if len(weights) != len(biases):
      raise ValueError('as many bias vectors as weight matrices, got %d and %d'
                       % (len(biases), len(weights)))
    if len(weights) not in (2, 3):
      raise ValueError('1 or 2 hidden layers (2 or 3 weight matrices), got %d matrices'
                       % len(weights))
    for l, (w, b) in enumerate(zip(weights, biases)):
      if w.ndim != 2 or 0 in w.shape:
        raise ValueError('weights[%d] must be a matrix [out, in], got shape %r' % (l, w.shape))
      if b.shape != (w.shape[0],):
        raise ValueError('biases[%d] must have shape (%d,), got %r' % (l, w.shape[0], b.shape))
      if l and w.shape[1] != weights[l - 1].shape[0]:
        raise ValueError('weights[%d] takes %d inputs, layer %d puts out %d'
                         % (l, w.shape[1], l - 1, weights[l - 1].shape[0]))
    self.weights, self.biases = weights, biases
    self.version = 0        # counts `update_` calls: device copies are cached per version

  @property
  def obs_dim(self):
    return self.weights[0].shape[1]

  @property
  def action_dim(self):
    return self.weights[-1].shape[0]

  @property
  def widths(self):
    """Hidden widths, then the output width."""
    return tuple(w.shape[0] for w in self.weights)

  @classmethod
  def from_torch(cls, module):
    """From an `nn.Sequential` of Linear, Tanh, [Linear, Tanh,] Linear."""
    import torch  # pylint: disable=g-import-not-at-top
    layers = list(module)
    weights, biases = [], []
    for k, layer in enumerate(layers):
      if k % 2 == 0:
        if not isinstance(layer, torch.nn.Linear):
          raise ValueError('layer %d must be nn.Linear, got %s' % (k, type(layer).__name__))
        weights.append(layer.weight.detach().cpu().double().numpy())
        biases.append(np.zeros(layer.out_features) if layer.bias is None
                      else layer.bias.detach().cpu().double().numpy())
      elif not isinstance(layer, torch.nn.Tanh):
        raise ValueError('layer %d must be nn.Tanh, got %s' % (k, type(layer).__name__))
    if len(layers) % 2 == 0:
      raise ValueError('the last layer must be nn.Linear (a linear output)')
    return cls(weights, biases)

  def update_(self, weights, biases):
    """New values, same shapes; device copies are uploaded again on next use."""
    new = MLPPolicy(weights, biases)
    if new.widths != self.widths or new.obs_dim != self.obs_dim:
      raise ValueError('update_ keeps the shapes: %r from %d inputs'
                       % (self.widths, self.obs_dim))
    self.weights, self.biases = new.weights, new.biases
    self.version += 1
    return self

  def packed(self, dtype):
    """The flat array the kernel reads: per layer W row-major, then b."""
    return np.concatenate([np.concatenate([w.ravel(), b])
                           for w, b in zip(self.weights, self.biases)]).astype(dtype)

  @classmethod
  def unpacked(cls, flat, obs_dim, widths):
    """Inverse of `packed`."""
    flat = np.asarray(flat, np.float64)
    weights, biases, at, fan_in = [], [], 0, obs_dim
    ins = (obs_dim,) + tuple(widths[:-1])
    if flat.ndim != 1 or flat.size != sum(o*(i + 1) for i, o in zip(ins, widths)):
      raise ValueError('%d values for widths %r from %d inputs, which take %d'
                       % (flat.size, tuple(widths), obs_dim,
                          sum(o*(i + 1) for i, o in zip(ins, widths))))
    for out in widths:
      weights.append(flat[at:at + out*fan_in].reshape(out, fan_in))
      at += out*fan_in
      biases.append(flat[at:at + out])
      at += out
      fan_in = out
    return cls(weights, biases)

  def forward(self, obs, dtype=None, tanh_ulps=0.0):
    """fp64 model of the policy on obs [..., obs_dim].

    dtype None: the actions.  Else (actions, bound): the weights are first rounded
    to `dtype` (what the device holds) and `bound` is the first-order forward
    error bound, elementwise, of evaluating in `dtype` with unit roundoff u: per
    layer (fan_in + 1) u (|W| |h| + |b|) for the dot products, |W| dh for the
    incoming error, and tanh passing errors on with Lipschitz constant 1 while
    adding tanh_ulps*u itself."""
    h = np.asarray(obs, np.float64)
    if dtype is None:
      for l, (w, b) in enumerate(zip(self.weights, self.biases)):
        h = h @ w.T + b
        if l < len(self.weights) - 1:
          h = np.tanh(h)
      return h
    u = float(np.finfo(dtype).eps)/2
    dh = np.zeros_like(h)
    for l, (w, b) in enumerate(zip(self.weights, self.biases)):
      w = w.astype(dtype).astype(np.float64)
      b = b.astype(dtype).astype(np.float64)
      dh = (w.shape[1] + 1)*u*(np.abs(h) @ np.abs(w).T + np.abs(b)) + dh @ np.abs(w).T
      h = h @ w.T + b
      if l < len(self.weights) - 1:
        h = np.tanh(h)
        dh = dh + tanh_ulps*u
    return h, dh


def _nparams(obs_dim, widths):
  ins = (obs_dim,) + tuple(widths[:-1])
  return sum(o*(i + 1) for i, o in zip(ins, widths))


class MLPPopulation:
  """P policies of one shape, held as `theta` [P, nparams] (fp64 on the host): row i
  is `member(i).packed`.  Or, from `from_device`, a CUDA tensor [nparams, P] that the
  kernel reads in place and the caller updates in place."""

  def __init__(self, theta, obs_dim, widths, device_tensor=None):
    self.obs_dim = int(obs_dim)
    self.widths = tuple(int(w) for w in widths)
    if len(self.widths) not in (2, 3) or min(self.widths) < 1 or self.obs_dim < 1:
      raise ValueError('1 or 2 hidden layers and an output layer of at least one unit '
                       'each, got widths %r from %d inputs' % (self.widths, self.obs_dim))
    self.nparams = _nparams(self.obs_dim, self.widths)
    self.device_tensor = device_tensor
    self.version = 0        # counts `update_` calls: device copies are cached per version
    if device_tensor is not None:
      self.theta = None
      self.num_members = int(device_tensor.shape[1])
    else:
      self.theta = self._checked(theta, None)
      self.num_members = self.theta.shape[0]

  def _checked(self, theta, members):
    theta = np.array(theta, np.float64)
    if theta.ndim != 2 or theta.shape[0] < 1 or theta.shape[1] != self.nparams or (
        members is not None and theta.shape[0] != members):
      raise ValueError('theta must have shape (%s, %d) for widths %r from %d inputs, got %r'
                       % ('P' if members is None else members, self.nparams, self.widths,
                          self.obs_dim, theta.shape))
    return theta

  @property
  def action_dim(self):
    return self.widths[-1]

  @classmethod
  def from_flat(cls, theta, obs_dim, widths):
    """theta [P, nparams]: row i is member i in the packed order of `MLPPolicy`."""
    return cls(theta, obs_dim, widths)

  @classmethod
  def from_policies(cls, policies):
    policies = list(policies)
    if not policies:
      raise ValueError('a population has at least one member')
    first = policies[0]
    for i, p in enumerate(policies):
      if p.widths != first.widths or p.obs_dim != first.obs_dim:
        raise ValueError('members of a population have one shape: member %d has widths %r '
                         'from %d inputs, member 0 %r from %d'
                         % (i, p.widths, p.obs_dim, first.widths, first.obs_dim))
    return cls(np.stack([p.packed(np.float64) for p in policies]), first.obs_dim, first.widths)

  @classmethod
  def from_device(cls, tensor, obs_dim, widths):
    """Wraps a C-contiguous CUDA tensor [nparams, P] of the code object's dtype: the
    kernel reads it in place (no upload, no copy), and what the caller writes into it
    -- an ES update, on the device -- is what the next rollout acts with."""
    pop = cls(None, obs_dim, widths, device_tensor=tensor)
    if (tensor.dim() != 2 or tensor.shape[0] != pop.nparams or tensor.shape[1] < 1
        or not tensor.is_cuda or not tensor.is_contiguous()):
      raise ValueError('expected a contiguous CUDA tensor [%d, P] for widths %r from %d '
                       'inputs, got %r' % (pop.nparams, pop.widths, pop.obs_dim,
                                           tuple(tensor.shape)))
    return pop

  def _host(self):
    if self.theta is None:
      return self.device_tensor.detach().cpu().double().numpy().T
    return self.theta

  def member(self, i):
    """Member i as an `MLPPolicy` (a copy)."""
    return MLPPolicy.unpacked(np.array(self._host()[i]), self.obs_dim, self.widths)

  def update_(self, theta):
    """New values [P, nparams], same shape; device copies are uploaded again on next
    use.  (A `from_device` population is updated by writing its tensor.)"""
    if self.theta is None:
      raise ValueError('a from_device population is updated in place, through its tensor')
    self.theta = self._checked(theta, self.num_members)
    self.version += 1
    return self

  def packed(self, dtype):
    """What the kernel reads: [nparams, P], C-contiguous; column i is
    `member(i).packed(dtype)`."""
    return np.ascontiguousarray(self._host().T.astype(dtype))
