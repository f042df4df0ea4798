// The host side of the XBL filter's entry points -- the `-filter` option (host/renderer_interface.h, parse_filter_option), what fpt_xbl refuses before it launches and the
// FPT_XBL_LAYOUT variable (fpt_host.h: xbl_check_args, xbl_layout_from) -- as a stand-alone CPU program, to be built with -fsanitize=address,undefined:
//   bash tools/sanitize_xbl_host.sh
#include "fpt_host.h"
#include "host/renderer_interface.h"
#include <cstdio>
#include <string>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); ++failures; } } while (0)

template <class F> static std::string refusal(F f)
{
	try { f(); } catch (const std::exception& e) { return e.what(); }
	return "";
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main()
{
	using fermat::parse_filter_option;
	CHECK(parse_filter_option("eaw") == 0u && parse_filter_option("xbl") == 1u);
	CHECK(has(refusal([] { parse_filter_option("median"); }), "-filter median"));
	CHECK(has(refusal([] { parse_filter_option(""); }), "-filter"));
	CHECK(has(refusal([] { parse_filter_option(nullptr); }), "expected eaw or xbl"));          // `-filter` as the last argument
	CHECK(has(refusal([] { parse_filter_option("xbl "); }), "-filter xbl "));
	CHECK(has(refusal([] { parse_filter_option(std::string(5000, 'x').c_str()); }), "expected eaw or xbl"));

	float a[4] = { 0 }, b[4] = { 0 }, g[4] = { 0 }, w[4] = { 0 }, sh[2] = { 0 };
	fpt_xbl_params p = {};
	CHECK(refusal([&] { xbl_check_args(a, b, g, &p, nullptr, 0x20u, sh, 1u); }).empty());
	CHECK(refusal([&] { xbl_check_args(a, b, g, &p, nullptr, 0x10u, sh, 256u); }).empty());
	CHECK(refusal([&] { xbl_check_args(a, b, g, &p, w, 0x16u, sh, 0x80000000u); }).empty());
	CHECK(has(refusal([&] { xbl_check_args(nullptr, b, g, &p, w, 0u, sh, 8u); }), "null buffer"));
	CHECK(has(refusal([&] { xbl_check_args(a, nullptr, g, &p, w, 0u, sh, 8u); }), "null buffer"));
	CHECK(has(refusal([&] { xbl_check_args(a, b, nullptr, &p, w, 0u, sh, 8u); }), "null buffer"));
	CHECK(has(refusal([&] { xbl_check_args(a, b, g, nullptr, w, 0u, sh, 8u); }), "null buffer"));
	CHECK(has(refusal([&] { xbl_check_args(a, b, g, &p, w, 0u, nullptr, 8u); }), "d_shifts is NULL"));
	for (uint32_t t : { 0u, 3u, 6u, 255u, 257u, 0xffffffffu })
		CHECK(has(refusal([&] { xbl_check_args(a, b, g, &p, w, 0u, sh, t); }), "tile_size must be a power of two"));
	for (uint32_t op : { 0x1u, 0x2u, 0x4u, 0x8u, 0x16u })
		CHECK(has(refusal([&] { xbl_check_args(a, b, g, &p, nullptr, op, sh, 8u); }), "needs a weight image"));
	CHECK(has(refusal([&] { xbl_check_args(a, a, g, &p, w, 0u, sh, 8u); }), "dst must not alias img"));

	CHECK(xbl_layout_from(nullptr) == 3 && xbl_layout_from("") == 3);
	CHECK(xbl_layout_from("0") == 0 && xbl_layout_from("1") == 1 && xbl_layout_from("2") == 2 && xbl_layout_from("3") == 3);
	for (const char* bad : { "4", "7", "-1", "10", "1 ", "x", "\xff" })
		CHECK(has(refusal([&] { xbl_layout_from(bad); }), "FPT_XBL_LAYOUT"));

	std::printf(failures ? "xbl_host_check: %d FAILED\n" : "xbl_host_check: ok\n", failures);
	return failures ? 1 : 0;
}
