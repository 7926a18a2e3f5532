// Boost stand-in for the build of the reference's consumer (oracle/Makefile, ref_consumer), so that it needs no Boost:
// boost::lexical_cast<std::string>(integer | double),
// double printed with 17 significant digits like Boost does (contig.cpp:1006 "avgDepth: 22.271739130434781")
#pragma once
#include <cstdio>
#include <string>
#include <type_traits>
namespace boost {
template <class To, class From> To lexical_cast(const From &v)
{
	static_assert(std::is_same<To, std::string>::value, "stand-in: only lexical_cast<std::string>");
	char buf[64];
	if (std::is_floating_point<From>::value) snprintf(buf, sizeof buf, "%.17g", (double)v);
	else if (std::is_signed<From>::value) snprintf(buf, sizeof buf, "%lld", (long long)v);
	else snprintf(buf, sizeof buf, "%llu", (unsigned long long)v);
	return std::string(buf);
}
}
