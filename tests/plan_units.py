"""Device-side helpers shared by the GPU tests that walk a compiled CVAE plan (plain module, no test in here):
test_gpu_parity_r3.py (the fiducial network) and test_gpu_arch_sweep.py (the layer-language sweep)."""


def conv_units(plan):
    """Every unit of a plan in execution order, residual blocks replaced by the units of their branches."""
    out = []

    def walk(us):
        for u in us:
            if hasattr(u, "body"):
                walk(u.body)
            else:
                out.append(u)
    for us in plan.q_units:
        walk(us)
    walk(plan.p_units)
    walk(getattr(plan, "y_units", []))
    for us in plan.g_units:
        walk(us)
    walk(plan.mu_units)
    walk(plan.var_units)
    return out


def residual_units(plan):
    """The residual blocks of a plan (units with a ``body``), nested ones included."""
    out = []

    def walk(us):
        for u in us:
            if hasattr(u, "body"):
                out.append(u)
                walk(u.body)
    for us in list(plan.q_units) + [plan.p_units, getattr(plan, "y_units", [])] + list(plan.g_units) \
            + [plan.mu_units, plan.var_units]:
        walk(us)
    return out


def raw_of(slot):
    """A slot's stored tensor as float32 NCHW on the host."""
    return slot.buf[..., slot.coff:slot.coff + slot.c].permute(0, 3, 1, 2).float().cpu()


def grad_of(slot):
    """What the backward pass left in a slot's gradient buffer (a channel slice of the wide buffer, or the dense buffer
    of a slice that keeps its own), as float32 NCHW on the host."""
    g = slot.grad_buf
    g = g if g.shape[-1] == slot.c and slot.cstride != slot.c else g[..., slot.coff:slot.coff + slot.c]
    return g.permute(0, 3, 1, 2).float().cpu()


def statistic_free_units(plan):
    """Names of the convolution units whose raw output depends on no batch-norm statistic: those with no batch-norm
    layer anywhere upstream (the recognition branches feed q_out, q_out the latent and p_z_in, p_z_in and p_y_in the
    trunk, the trunk the heads).  Two executions that differ only in HOW the statistics are summed agree bit for bit
    on these; behind a batch-norm layer they may differ by the rounding of its fp32 scale and shift."""
    free = set()

    def chain(units, dirty):
        for u in conv_units_of(units):
            if not dirty:
                free.add(u.name)
            dirty = dirty or getattr(u, "bn", None) is not None
        return dirty
    ux, uy, uo = plan.q_units if plan.q_units else ([], [], [])
    dq = chain(uo, chain(ux, False) | chain(uy, False))
    chain(plan.p_units, False)
    dy = chain(getattr(plan, "y_units", []), False)
    dt = chain(plan.g_units[1], chain(plan.g_units[0], dq) | dy)
    chain(plan.mu_units, dt)
    chain(plan.var_units, dt)
    return free


def conv_units_of(units):
    out = []
    for u in units:
        out += conv_units_of(u.body) if hasattr(u, "body") else [u]
    return out
