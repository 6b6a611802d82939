"""functional.linear_adjoint on the CPU: the core every linear PDE-layer node routes its backward through in grad mode.

The toy layer is y = A(theta) u with A = diag(exp(a)) + b c^T.  Its forward and its backward are computed under ``no_grad``
— as the library's kernels compute into fresh buffers — so torch cannot see through either; only the core makes
``autograd.grad(..., create_graph=True)`` differentiable.  For a cotangent v on gu = A^T g:  <v, A^T g> = <A v, g>, so the
gradient with respect to g is the layer at v and the gradient with respect to theta is the parameter gradient of the layer at
v with cotangent g."""
import pytest
import torch


def _A(a, b, c):
    return torch.diag(torch.exp(a)) + torch.outer(b, c)


def _toy():
    from cnn_with_pde_amd import functional as F

    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, u, a, b, c):
            ctx.save_for_backward(u, a.detach(), b.detach(), c.detach())
            ctx.primal_args = ((a, b, c), ())
            ctx.runs = 0
            with torch.no_grad():
                return u @ _A(a, b, c).T

        @staticmethod
        def _backward(ctx, g):
            u, a, b, c = ctx.saved_tensors
            ctx.runs += 1
            with torch.no_grad():
                gu = g @ _A(a, b, c)
                gA = g.T @ u                                  # dL/dA[i, j] = sum_n g[n, i] u[n, j]
                return gu, torch.diagonal(gA) * torch.exp(a), gA @ c, gA.T @ b

        @staticmethod
        def backward(ctx, g):
            if torch.is_grad_enabled():
                return F._second_order(Toy, ctx, (g,))
            return Toy._backward(ctx, g)

    return Toy


def _inputs(n=4, B=3, seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    u, g = r(B, n).requires_grad_(True), r(B, n).requires_grad_(True)
    a, b, c = (0.3 * r(n)).requires_grad_(True), r(n).requires_grad_(True), r(n).requires_grad_(True)
    return u, g, a, b, c


def test_the_toy_layer_is_opaque_to_torch_and_right_at_first_order():
    Toy = _toy()
    u, g, a, b, c = _inputs()
    assert torch.autograd.gradcheck(Toy.apply, (u, a, b, c))
    y = Toy.apply(u, a, b, c)
    (gu,) = torch.autograd.grad(y, u, g.detach())             # create_graph=False: the bare body, no graph on gu
    assert gu.grad_fn is None and torch.allclose(gu, g.detach() @ _A(a, b, c).detach())


def test_gradcheck_of_the_input_gradient_in_the_cotangent_and_the_parameters():
    Toy = _toy()
    u, g, a, b, c = _inputs()

    def phi(g, a, b, c):
        return torch.autograd.grad(Toy.apply(u, a, b, c), u, g, create_graph=True)[0]

    assert phi(g, a, b, c).grad_fn is not None
    assert torch.autograd.gradcheck(phi, (g, a, b, c))
    # ... and against what torch gives for the transparent layer
    v = torch.randn(3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    got = torch.autograd.grad(phi(g, a, b, c), (g, a, b, c), v)
    want = torch.autograd.grad(torch.autograd.grad(u @ _A(a, b, c).T, u, g, create_graph=True)[0], (g, a, b, c), v)
    for x, y in zip(got, want):
        assert torch.allclose(x, y, rtol=1e-12, atol=1e-12)
    assert torch.autograd.gradgradcheck(lambda x: Toy.apply(x, a.detach(), b.detach(), c.detach()), (u,))
    assert torch.autograd.gradgradcheck(Toy.apply, (u, a.detach(), b.detach(), c.detach()))


def test_a_cotangent_on_a_parameter_gradient_raises():
    Toy = _toy()
    u, g, a, b, c = _inputs()
    gu, ga = torch.autograd.grad(Toy.apply(u, a, b, c), (u, a), g, create_graph=True)
    assert ga.grad_fn is not None                             # looks differentiable, so that it can refuse aloud
    torch.autograd.grad(gu.sum(), (g, a), retain_graph=True)  # the input gradient alone is fine
    with pytest.raises(NotImplementedError, match="not differentiable"):
        torch.autograd.grad(ga.sum(), g, retain_graph=True)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        (gu.sum() + ga.sum()).backward()


def test_third_order():
    Toy = _toy()
    u, g, a, b, c = _inputs()
    v = torch.randn(3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).requires_grad_(True)

    def psi(layer):
        def f(g, v, a, b, c):
            gu = torch.autograd.grad(layer(u, a, b, c), u, g, create_graph=True)[0]
            return torch.autograd.grad(gu, g, v, create_graph=True)[0]      # = layer(v): differentiable once more
        return f

    got = psi(Toy.apply)(g, v, a, b, c)
    assert got.grad_fn is not None and torch.allclose(got, v @ _A(a, b, c).T)
    assert torch.autograd.gradcheck(psi(Toy.apply), (g, v, a, b, c))
    w = torch.randn(3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    third = torch.autograd.grad(got, (v, a, b, c), w)
    want = torch.autograd.grad(psi(lambda u, a, b, c: u @ _A(a, b, c).T)(g, v, a, b, c), (v, a, b, c), w)
    for x, y in zip(third, want):
        assert torch.allclose(x, y, rtol=1e-12, atol=1e-12)


def test_a_retained_graph_runs_the_first_order_backward_again():
    Toy = _toy()
    u, g, a, b, c = _inputs()
    y = Toy.apply(u, a, b, c)
    (gu,) = torch.autograd.grad(y, u, g.detach(), create_graph=True)
    ctx = y.grad_fn
    assert ctx.runs == 1
    (y.sum() + 0.0 * gu.pow(2).sum()).backward()
    assert ctx.runs == 2                                      # the primal node was walked a second time, bare
    ref = _inputs()
    Toy.apply(*[ref[i] for i in (0, 2, 3, 4)]).sum().backward()
    for x, r in zip((u, a, b, c), (ref[0], ref[2], ref[3], ref[4])):
        assert torch.equal(x.grad, r.grad)


def test_missing_cotangents_and_missing_parameters_pass_through():
    from cnn_with_pde_amd import functional as F
    s = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    g = torch.randn(5, dtype=torch.float64, requires_grad=True)

    def body(c):
        return c * s.detach(), c * (1 - s.detach()), None

    def primal(v0, v1):
        z = torch.zeros(5, dtype=torch.float64)
        return (z if v0 is None else v0) * s + (z if v1 is None else v1) * (1 - s)

    ga, gb, gw = F.linear_adjoint(body, primal, (g,), (s, None), n_diff=2)
    assert gw is None
    v = torch.randn(5, dtype=torch.float64)
    gg, gs = torch.autograd.grad(ga, (g, s), v)               # gb takes no cotangent
    assert torch.allclose(gg, v * s) and torch.allclose(gs, (v * g).sum())
