"""What the two glue test modules share (tests/test_agent_glue_host.py, tests/test_step_glue_host.py): the central-difference
check with the scheme's own error estimate and the did-this-comparison-fail helper.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

f64 = np.float64


def fd_check(loss_rows, x, analytic, name, h0=1e-4):
  """d (per-row loss) / d x[:, c] by central differences with steps h and h / 2.  The scheme's own error estimate: the
  truncation error of the h / 2 difference is a third of |D(h) - D(h / 2)|; its rounding error 2^-52 |loss| / (h / 2)."""
  x = np.asarray(x, dtype=f64)
  base = np.abs(loss_rows(x))
  for c in range(x.shape[1]):
    h = h0 * max(1.0, float(np.abs(x[:, c]).max()))
    d = []
    for step in (h, h / 2):
      e = np.zeros_like(x)
      e[:, c] = step
      d.append((loss_rows(x + e) - loss_rows(x - e)) / (2 * step))
    bound = np.abs(d[0] - d[1]) + 2.0**-50 * (base + 1e-300) / (h / 2) + 1e-300
    err = np.abs(analytic[:, c] - d[1])
    assert (err <= bound).all(), (name, c, float((err / bound).max()))
    # ... and the estimate is tight enough to tell a 0.1 % error wherever the derivative is not itself negligible
    big = np.abs(analytic[:, c]) > 1e-3 * np.abs(analytic).max()
    assert (bound[big] <= 1e-3 * np.abs(analytic[big, c])).all(), (name, c)


def rejected(check, got):
  try:
    check(got)
  except AssertionError:
    return True
  return False
