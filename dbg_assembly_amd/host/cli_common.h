// cli_common.h -- what every command-line program here uses: die() on a failed C call, the reference's split() and lib-file
// reader, gzip line input and output, and strings laid back to back for the device.
#pragma once
#include <zlib.h>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "dbgk.h"

using namespace std;

static void die(const char *what, int rc)
{
	cerr << what << " failed: " << dbgk_strerror(rc);
	if (rc == DBGK_ERR_HIP) cerr << " [" << dbgk_last_error() << "]";
	cerr << endl;
	exit(1);
}

// split (map_func.cpp:33-53, the same in link_func.cpp)
[[maybe_unused]] static void split(const string &line, vector<string> &tokens, const char *delim)
{
	size_t i = 0;
	for (;;) {
		i = line.find_first_not_of(delim, i);
		if (i == string::npos) break;
		const size_t j = line.find_first_of(delim, i);
		tokens.push_back(line.substr(i, j == string::npos ? string::npos : j - i));
		if (j == string::npos) break;
		i = j;
	}
}

// reading_lib_file (map_func.cpp:57-77) and reading_para_file (link_func.cpp:75-95): '#' lines and empty lines skipped, the first
// token taken
[[maybe_unused]] static void reading_lib_file(const string &lib_file, vector<string> &files)
{
	ifstream infile(lib_file.c_str());
	if (!infile) cerr << "fail to open input file" << lib_file << endl;
	string line;
	while (getline(infile, line, '\n')) {
		if (!line.empty() && line[0] == '#') continue;
		vector<string> vec_line;
		split(line, vec_line, " \t\n");
		if (vec_line.empty()) continue;
		files.push_back(vec_line[0]);
	}
}

// getline over a plain or gzip file (what igzstream + getline read); a caller with a message of its own for a failed open
// passes report = false and asks ok()
struct LineReader {
	gzFile f = nullptr;
	vector<char> buf = vector<char>(1 << 20);
	size_t pos = 0, len = 0;
	bool eof = false;
	explicit LineReader(const string &path, bool report = true)
	{
		f = gzopen(path.c_str(), "rb");
		if (f) gzbuffer(f, 1 << 20);
		else if (report) cerr << "fail to open input file " << path << endl;
	}
	~LineReader() { if (f) gzclose(f); }
	bool ok() const { return f != nullptr; }
	bool getline(string &s)
	{
		s.clear();
		bool any = false;
		for (;;) {
			if (pos == len) {
				if (eof || !f) return any;
				const int n = gzread(f, buf.data(), (unsigned)buf.size());
				if (n <= 0) { eof = true; return any; }
				pos = 0;
				len = (size_t)n;
			}
			any = true;
			const char *b = buf.data() + pos;
			const char *nl = (const char *)memchr(b, '\n', len - pos);
			if (nl) {
				s.append(b, nl - b);
				pos += (nl - b) + 1;
				return true;
			}
			s.append(b, len - pos);
			pos = len;
		}
	}
};

// what ogzstream writes
struct GzWriter {
	gzFile f = nullptr;
	explicit GzWriter(const string &path)
	{
		f = gzopen(path.c_str(), "wb");
		if (!f) cerr << "fail to open output file " << path << endl;
	}
	~GzWriter() { if (f) gzclose(f); }
	void write(const string &s)
	{
		if (f && !s.empty()) gzwrite(f, s.data(), (unsigned)s.size());
	}
};

// the strings of v back to back, string i at bases[offsets[i] .. offsets[i + 1])
[[maybe_unused]] static void concat(const vector<string> &v, string &bases, vector<uint64_t> &offsets)
{
	bases.clear();
	offsets.assign(1, 0);
	for (const string &s : v) {
		bases += s;
		offsets.push_back(bases.size());
	}
}
